"""tone8 without a GPU: the numpy restatement in
tests/tone8_cases.py (the checker of the GPU kernels) is itself a working
modem -- it recovers its own frames, aligned, from random delays with the
receiver tuned up to G half tone spacings off the sender, at every valid
geometry of up to 40 samples per symbol, and under noise --, its rules are
total, the geometry's limits are refused on the host, and the C ABI refuses
bad arguments before any device work."""
import ctypes

import numpy as np
import pytest

import spread_cases as sp
import tone8_cases as tc

TRIALS = 12
# (baud, carrier, search) at 96 kHz: c2 = 5, 5 and 40, so 3 is the widest search the first two admit
CONFIGS = [(1200, 3000.0, 3), (600, 1500.0, 3), (50, 1000.0, 6)]
# test_noise: per configuration the largest sigma of the ladder 0.25, 0.5 .. 3.0 at which the restatement returns
# every one of the 12 seeded payloads (the scan is in the docstring); the test asserts one ladder step below it
CLEARED = {1200: 1.0, 600: 1.5, 50: 3.0}
STEP = 0.25


@pytest.fixture(scope="module")
def product(built_lib):
    """The restatement is only worth testing beside the product it restates."""
    import _amr
    import modem
    for name in ("tone8_modulate", "tone8_demodulate", "tone8_demodulate_batch", "tone8_demodulate_soft",
                 "tone8_demodulate_soft_batch", "tone8_acquire", "tone8_acquire_batch"):
        assert callable(getattr(modem, name)), name
    for name in ("tone8_geometry", "design_tone8", "Tone8Plan", "get_tone8_plan", "tone8_tx_samples", "tone8_modulate",
                 "tone8_peak", "tone8_slice", "tone8_soft", "tone8_chunk"):
        assert callable(getattr(_amr, name)), name
    assert _amr.Tone8Plan._slots == _amr.TD_SLOTS == ["despread", "slice", "sync_pack", "launch", "acquire"]
    return _amr.lib()


def payload(rng, n):
    return b"FBPC" + rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def recovered(data, sync, msg):
    """The sync word was found and the payload follows it (what lies behind it is padding and the tail)."""
    return sync >= 0 and data[:len(msg)] == msg


def circ(start, t, L):
    return min((start - t) % L, (t - start) % L)


def test_geometry_and_the_frame(product):
    import _amr
    g = _amr.tone8_geometry
    assert g(1200, 3000.0, 96000, 3) == (80, 10, 5, 3) and g(50, 1000.0) == (1920, 240, 40, 6)
    assert g(600, 1500.0, 96000, 0) == (160, 20, 5, 0) and g(*tc.pair_of(24, 3), 1) == (24, 3, 3, 1)
    assert _amr.TONE8_COSTAS == (3, 1, 4, 0, 6, 5, 2)
    # a Costas array: the 21 difference vectors between its marks are distinct
    c = _amr.TONE8_COSTAS
    assert len({(b - a, c[b] - c[a]) for a in range(7) for b in range(a + 1, 7)}) == 21
    assert [int(t) for t in tc.GRAY] == [0, 1, 3, 2, 6, 7, 5, 4] and all(tc.UNGRAY[tc.GRAY[v]] == v for v in range(8))
    msg = b"\xe5\x01"                                        # 111 001 010 000 000 1(00): tribits 7, 1, 2, 0, 0, 4
    assert tc.tx_tones(msg).tolist() == [3, 1, 4, 0, 6, 5, 2] + [4, 1, 3, 0, 0, 6]
    assert _amr.tone8_tx_samples(2, 1200, 3000.0) == 13 * 80 == tc.modulate(msg, 1200, 3000.0).size
    assert _amr.tone8_tx_samples(0, 1200, 3000.0) == 7 * 80 and _amr.tone8_tx_samples(3, 1200, 3000.0) == 15 * 80


def test_invalid_geometries(product):
    import _amr
    import modem
    g = _amr.tone8_geometry
    bad = [
        dict(baud=1100),                                     # L = 87, not a multiple of 8
        dict(baud=6000), dict(baud=12000), dict(baud=200000),   # L = 16 (c2 + 14 >= L at any c2 >= 2), 8, 0
        dict(carrier=3000.0, search=4),                      # c2 - G = 1
        dict(carrier=600.0, search=0),                       # c2 = 1
        dict(carrier=37800.0, search=3),                     # c2 = 63: 63 + 14 + 3 = 80 = L
        dict(search=17), dict(search=-1), dict(search=2.5),
        dict(baud=0.001),                                    # L > 2^24
    ]
    assert g(1000, 3000.0, 96000, 3)[0] == 96 and g(1200, 37200.0, 96000, 3)[2] == 62      # 62 + 17 = 79: the last valid
    for kw in bad:
        args = dict(baud=1200, carrier=3000.0, search=3)
        args.update(kw)
        b, c, s = args["baud"], args["carrier"], args["search"]
        with pytest.raises(ValueError):
            g(b, c, 96000, s)
        with pytest.raises(ValueError):                      # before any device work: no GPU is needed to refuse
            modem.tone8_demodulate(np.zeros(4000, np.float32), b, c, search=s)
        with pytest.raises(ValueError):
            modem.tone8_acquire_batch(np.zeros((0, 10), np.float32), b, c, search=s)
        with pytest.raises(ValueError):
            modem.tone8_demodulate_soft_batch(np.zeros((0, 10), np.float32), b, c, search=s)
    for b, c in ((1100, 3000.0), (6000, 12000.0), (1200, 600.0), (1200, 40000.0)):   # the modulator: the geometry at G = 0
        with pytest.raises(ValueError):
            modem.tone8_modulate(b"x", b, c)
        with pytest.raises(ValueError):
            modem.modulate_batch("tone8", [b"x"], b, c)
    # the C side refuses the same before any device work
    L = product
    h = ctypes.c_void_p()
    E = _amr.design_tone8(1200, 3000.0, 96000, 3)[5]
    p = _amr.ptr
    inv = _amr.AMR_E_INVALID
    create = L.amr_tone8_plan_create
    assert create(ctypes.byref(h), 0, 1000, 87, 5, 3, p(E), 1) == inv
    assert create(ctypes.byref(h), 0, 1000, 16, 2, 0, p(E), 1) == inv
    assert create(ctypes.byref(h), 0, 1000, 80, 5, 4, p(E), 1) == inv
    assert b"lowest searched line" in L.amr_last_error()
    assert create(ctypes.byref(h), 0, 1000, 80, 63, 3, p(E), 1) == inv
    assert b"highest searched line" in L.amr_last_error()
    assert create(ctypes.byref(h), 0, 1000, 80, 20, 17, p(E), 1) == inv
    assert create(ctypes.byref(h), 0, 1000, 80, 20, -1, p(E), 1) == inv
    assert create(ctypes.byref(h), 0, 1000, (1 << 24) + 8, 40, 6, p(E), 1) == inv
    assert create(ctypes.byref(h), 0, -1, 80, 5, 3, p(E), 1) == inv
    assert create(ctypes.byref(h), 0, 1000, 80, 5, 3, p(E), 0) == inv
    assert create(ctypes.byref(h), 0, 1000, 80, 5, 3, None, 1) == inv
    assert create(None, 0, 1000, 80, 5, 3, p(E), 1) == inv


def round_trips(baud, carrier, fs, G, rng, n_payload, delays=2):
    """The aligned clean capture comes back exactly, sync at bit 21; from random delays below 5 L, digital silence
    before and 2 L after, with the sender a random number of half spacings off, a clean capture gives its
    payload, the shift exactly and the start within a slot of the delay."""
    L, T, c2, G = tc.geometry(baud, carrier, fs, G)
    msg = payload(rng, n_payload)
    w = tc.modulate(msg, baud, carrier, fs)
    assert w.dtype == np.float32 and w.size == (7 + -(-8 * len(msg) // 3)) * L
    data, sync, start, g = tc.demod(w, baud, carrier, fs, acquire_=False, search=G)
    assert (data[:len(msg)], sync, start, g) == (msg, tc.SYNC_AT, 0, 0), (L, c2)
    sdata, soft, ssync, _, _ = tc.demod_soft(w, baud, carrier, fs, acquire_=False, search=G)
    assert (sdata, ssync) == (data, sync) and np.packbits(soft > 0).tobytes() == data
    assert tc.acquire(w, baud, carrier, fs, G)[:2] == (0, 0)
    for _ in range(delays):
        t = int(rng.integers(0, 5 * L))
        off = int(rng.integers(-G, G + 1))
        x = tc.delayed(msg, t, baud, carrier, samp_rate=fs, off=off)
        assert x.size == t + w.size + 2 * L
        data, sync, start, g = tc.demod(x, baud, carrier, fs, search=G)
        assert g == off and circ(start, t, L) <= T and abs(start - t) <= T, (L, c2, t, off, start, g)
        assert recovered(data, sync, msg), (L, c2, t, off)


def test_every_valid_geometry_up_to_forty_samples_per_symbol(product):
    """Every (L, c2) with L in (24, 32, 40), 2 <= c2 and c2 + 14 < L at G = 0: aligned and from two delays, clean."""
    pairs = tc.valid_pairs(40)
    assert len(pairs) == 8 + 16 + 24 and (24, 2) in pairs and (24, 9) in pairs and (40, 25) in pairs
    assert not [p for p in pairs if p[0] == 8 or p[0] == 16]
    rng = np.random.default_rng(40)
    for L, c2 in pairs:
        round_trips(*tc.pair_of(L, c2), 0, rng, 8)


def test_the_smallest_symbol_and_its_searches(product):
    """L = 24 (T = 3): c2 - G >= 2 and c2 + 14 + G < 24 leave G <= 3, and G = 3 only c2 = 5 and 6."""
    import _amr
    rng = np.random.default_rng(24)
    for c2, G in ((3, 1), (4, 1), (8, 1), (4, 2), (5, 3), (6, 3)):
        round_trips(*tc.pair_of(24, c2), G, rng, 10, delays=4)
    for c2, G in ((4, 3), (7, 3), (6, 4), (2, 1), (9, 1)):
        with pytest.raises(ValueError):
            _amr.tone8_geometry(*tc.pair_of(24, c2), G)


def test_the_constant_envelope_and_the_continuous_phase(product):
    """Every sample is a table sine of one running integer phase, whose step from sample to sample is
    c2 + 2 tone units of 1 / (2 L) cycle, also across a symbol boundary; the tones are one symbol rate apart and
    orthogonal over a symbol."""
    import _amr
    baud, carrier = 1200, 3000.0
    L, T, c2, G, Sn, E = _amr.design_tone8(baud, carrier, 96000, 0)
    msg = payload(np.random.default_rng(1), 9)
    w = tc.modulate(msg, baud, carrier)
    tones = tc.tx_tones(msg)
    assert tones.size == 7 + -(-8 * len(msg) // 3) and set(tones.tolist()) <= set(range(8))
    inc = np.repeat(c2 + 2 * tones, L)
    phase = np.concatenate([[0], np.cumsum(inc)[:-1]]) % (2 * L)
    assert np.array_equal(w, Sn[phase].astype(np.float32))
    # the envelope: sin^2 + cos^2 of the same phase is 1
    quad = Sn[(phase + L // 2) % (2 * L)]
    assert np.abs(w.astype(np.float64) ** 2 + quad ** 2 - 1).max() < 1e-6
    f = (c2 + 2 * np.arange(8)) * 96000 / (2 * L)
    assert np.all(np.diff(f) == baud) and f[0] == carrier
    # orthogonal: a clean symbol of tone m puts (L / 2)^2 on its own line and nothing on the others
    Y = tc.symbols(w, 0, 0, baud, carrier, 96000, 0)
    e = tc.energies(Y)
    assert np.array_equal(np.argmax(e, axis=1), tones)
    own = e[np.arange(tones.size), tones]
    assert np.abs(own / (L / 2) ** 2 - 1).max() < 1e-6 and (e.sum(axis=1) - own).max() < 1e-6


@pytest.mark.parametrize("baud,carrier,G", CONFIGS + [tc.pair_of(24, 4)[:2] + (1,)])
def test_clean_captures(product, baud, carrier, G):
    """Delays below 5 L and 2 L of trailing zeros, the receiver tuned every number of half spacings from -G to G
    off the sender: the payload, shift == c2_tx - c2_rx exactly, start within one slot of the delay."""
    fs = tc.pair_of(24, 4)[2] if baud == 1000 else 96000
    L, T, c2, G = tc.geometry(baud, carrier, fs, G)
    rng = np.random.default_rng(int(baud) + 7)
    worst = 0
    for off in range(-G, G + 1):
        for _ in range(2):
            msg = payload(rng, int(rng.integers(8, 25)))
            t = int(rng.integers(0, 5 * L))
            x = tc.delayed(msg, t, baud, carrier, samp_rate=fs, off=off)
            c2_tx = tc.geometry(baud, carrier + off * baud / 2, fs, 0)[2]
            data, sync, start, g = tc.demod(x, baud, carrier, fs, search=G)
            assert recovered(data, sync, msg), (off, t)
            assert g == c2_tx - c2 == off, (off, t, g)
            worst = max(worst, circ(start, t, L))
            assert circ(start, t, L) <= L // 8 and abs(start - t) <= L // 8, (off, t, start)
            assert tc.acquire(x, baud, carrier, fs, G)[:2] == (start, g)
    print(f"tone8 clean {baud} Bd: worst timing error {worst} of a slot of {T}")


def test_off_grid_senders_are_measured(product):
    """A sender a quarter tone spacing from any grid line (np.sin, not the table): what the rule gives is printed,
    not required -- the rule refines no frequency.  Asserted: the result is one of the two neighbouring shifts."""
    baud, carrier, G = 1200, 3000.0, 3
    L, T, c2, _ = tc.geometry(baud, carrier, 96000, G)
    rng = np.random.default_rng(5)
    msg = payload(rng, 16)
    tones = tc.tx_tones(msg)
    got = []
    for quarter in (-5, -1, 1, 5):                           # the sender's carrier, in quarter spacings off the receiver's
        f = carrier + quarter * baud / 4 + tones * baud
        ph = 2 * np.pi * np.cumsum(np.repeat(f, L)) / 96000
        t = int(rng.integers(0, 5 * L))
        x = np.concatenate([np.zeros(t), np.sin(ph), np.zeros(2 * L)]).astype(np.float32)
        data, sync, start, g = tc.demod(x, baud, carrier, search=G)
        got.append((quarter, g, circ(start, t, L), recovered(data, sync, msg)))
        assert g in ((quarter - 1) // 2, (quarter + 1) // 2), got
    print("tone8 off-grid (quarter spacings, shift, timing error, payload back):", got)


def noisy_capture(baud, carrier, G, seed, sigma):
    rng = np.random.default_rng(1000 * seed + int(baud))
    msg = payload(rng, int(rng.integers(20, 61)))
    L = tc.geometry(baud, carrier, 96000, G)[0]
    t = int(rng.integers(0, 5 * L))
    off = int(rng.integers(-G, G + 1))
    return msg, t, off, tc.delayed(msg, t, baud, carrier, sigma=sigma, rng=rng, off=off)


@pytest.mark.parametrize("baud,carrier,G", CONFIGS)
def test_noise(product, baud, carrier, G):
    """Every one of the 12 seeded captures, delayed at random with the sender a random number of half spacings off,
    gives its payload back one ladder step below the largest sigma that cleared the scan.  Scan on the
    restatement (payloads / shifts exact / starts within a slot, of 12): 1200 Bd (L = 80) 12/12/12 from 0.25 to
    1.0, 5/12/11 at 1.25, 0/12/11 at 1.5, 0/10/9 at 2.0, 0/4/4 at 3.0 -> cleared 1.0; 600 Bd (L = 160) 12/12/12
    to 1.5, 7/11/12 at 1.75, 3/11/12 at 2.0, 0/10/12 at 2.25, 0/7/9 at 3.0 -> cleared 1.5; 50 Bd (L = 1920)
    12/12/12 at every rung to 3.0 -> cleared 3.0, the top of the ladder.  What fails first is the uncoded
    symbol decision, never the acquisition: the Costas score integrates seven symbols."""
    sigma = CLEARED[baud] - STEP
    L = tc.geometry(baud, carrier, 96000, G)[0]
    for seed in range(TRIALS):
        msg, t, off, x = noisy_capture(baud, carrier, G, seed, sigma)
        data, sync, start, g = tc.demod(x, baud, carrier, search=G)
        assert recovered(data, sync, msg), (seed, t, off, start, g)
        assert g == off and circ(start, t, L) <= L // 8, (seed, t, off, start, g)


def test_the_scan_rule_on_crafted_energies(product):
    """An exact tie in j, a tie in g, a NaN first candidate, a NaN elsewhere; the vectorised first maximum is the
    sequential rule."""
    nan = np.nan
    rng = np.random.default_rng(3)
    for _ in range(50):
        v = rng.integers(0, 4, 30).astype(np.float64)
        v[rng.integers(0, 30, 3)] = nan
        assert tc.first_max_flat(v) == sp.first_max(v)
    assert tc.first_max_flat(np.array([nan, 5.0])) == 0 and tc.first_max_flat(np.array([1.0, nan, 1.0, 2.0, 2.0])) == 3
    G, T = 2, 10
    NB = 15 + 2 * G

    def costas_at(P, j, g, v=1.0):
        for s in range(7):
            P[j + 8 * s, g + G + 2 * tc.COSTAS[s]] = v
    P = np.zeros((60, NB))
    assert tc.peak(P, T, G) == (0, -G, 0.0)                  # all equal: the first candidate
    costas_at(P, 5, 1)
    assert tc.peak(P, T, G) == (50, 1, 7.0)
    costas_at(P, 9, -2)                                      # the same score later in j: the first stays
    assert tc.peak(P, T, G) == (50, 1, 7.0)
    costas_at(P, 5, -1)                                      # and earlier in g at the same j: it wins
    assert tc.peak(P, T, G) == (50, -1, 7.0)
    Q = P.copy()
    Q[0, 2 * 3] = nan                                        # S[0][-G] reads P[0][2 costas[0]]: a NaN first candidate
    assert tc.peak(Q, T, G)[:2] == (0, -G) and np.isnan(tc.peak(Q, T, G)[2])
    Q = P.copy()
    Q[20, :] = nan                                           # NaN elsewhere never wins
    assert tc.peak(Q, T, G) == (50, -1, 7.0)
    Q = P.copy()
    costas_at(Q, 11, 2, np.inf)
    assert tc.peak(Q, T, G) == (110, 2, np.inf)
    assert tc.peak(np.zeros((48, NB)), T, G) == (0, 0, 0.0) and tc.peak(np.zeros((0, NB)), T, G) == (0, 0, 0.0)
    assert tc.peak(np.ones((49, NB)), T, G) == (0, -G, 7.0)


def test_the_rules_are_total(product):
    nan, inf = np.nan, np.inf
    baud, carrier, G = 1200, 3000.0, 3
    L, T, c2, _ = tc.geometry(baud, carrier, 96000, G)
    # n = 0, nj <= 0, all zeros
    for n in (0, 1, T - 1, 55 * T + T - 1, L - 1):
        x = np.ones(n, np.float32)
        assert tc.acquire(x, baud, carrier, search=G) == (0, 0, 0.0)
        data, sync, start, g = tc.demod(x, baud, carrier, search=G)
        assert (start, g) == (0, 0) and (n >= L or (data, sync) == (b"", -1))
    assert tc.demod(np.ones(L - 1, np.float32), baud, carrier, search=G)[:2] == (b"", -1)
    assert tc.demod_soft(np.ones(0, np.float32), baud, carrier, search=G)[:3:2] == (b"", -1)
    assert tc.acquire(np.zeros(56 * T, np.float32), baud, carrier, search=G) == (0, -G, 0.0)    # nj = 1, every score 0
    assert tc.acquire(np.zeros(5000, np.int16), baud, carrier, search=G) == (0, -G, 0.0)
    # a NaN or an infinity in the first start slot's windows is in S[0][-G]: (0, -G) is kept; later a NaN only
    # removes candidates
    rng = np.random.default_rng(9)
    msg = payload(rng, 20)
    x = tc.delayed(msg, 700, baud, carrier, off=-2)
    want = tc.acquire(x, baud, carrier, search=G)
    assert want[:2] == (700, -2)
    for k, v in ((0, nan), (3, inf), (79, -inf)):
        y = x.copy()
        y[k] = v
        with np.errstate(all="ignore"):
            s, g, sc_ = tc.acquire(y, baud, carrier, search=G)
        # an infinity makes the first score +inf (or a NaN where inf meets -inf): nothing is strictly greater
        assert (s, g) == (0, -G) and (np.isnan(sc_) if np.isnan(v) else not np.isfinite(sc_)), (k, v)
    y = x.copy()
    y[x.size - 5] = nan                                      # in the tail: the frame is still found
    with np.errstate(all="ignore"):
        assert tc.acquire(y, baud, carrier, search=G) == want
        assert tc.demod(y, baud, carrier, search=G)[2:] == (700, -2)
    # the decision and the soft values on special energies
    vals = [0.0, -0.0, 1.0, -1.0, 2.0 ** 600, 2.0 ** -600, 5e-324, inf, -inf, nan]
    Y = np.zeros((len(vals) ** 2, 8), np.complex128)
    Y[:, 0] = 0.5
    Y[:, 3] = [complex(a, b) for a in vals for b in vals]
    with np.errstate(all="ignore"):
        tones, bits, soft = tc.decide(Y), tc.slice_bits(Y), tc.soft(Y)
    assert set(tones.tolist()) == {0, 3} and bits.size == 3 * len(Y) and soft.dtype == np.int8
    assert np.array_equal(soft > 0, bits == 1) and np.all((np.abs(soft.astype(int)) >= 1) & (np.abs(soft.astype(int)) <= 127))
    e3 = tc.energies(Y)[:, 3]
    assert np.array_equal(tones == 3, e3 > 0.25) and not np.any(tones[np.isnan(e3)])
    Z = np.full((1, 8), complex(nan, 0.0))                   # every energy NaN: tone 0, magnitude 1
    with np.errstate(all="ignore"):
        assert tc.decide(Z).tolist() == [0] and tc.soft(Z).tolist() == [-1, -1, -1]
    Z = np.zeros((2, 8), np.complex128)                      # an exact tie of all eight: tone 0; of two: the lower
    Z[1, 2] = Z[1, 6] = 3.0
    assert tc.decide(Z).tolist() == [0, 2] and tc.soft(Z)[:3].tolist() == [-1, -1, -1]
    assert tc.slice_bits(np.zeros((0, 8), np.complex128)).size == 0 and tc.soft(np.zeros((0, 8), np.complex128)).size == 0


def test_the_summation_order_is_part_of_the_definition(product):
    """A slot sum is sequential in i, a window the fixed tree of its eight slots, a symbol four interleaved partials."""
    import _amr
    baud, carrier, G = 1200, 3000.0, 3
    L, T, c2, _, Sn, E = _amr.design_tone8(baud, carrier, 96000, G)
    rng = np.random.default_rng(2)
    x = rng.standard_normal(20 * T + 3)
    zr, zi = tc.slot_sums(x, baud, carrier, search=G)
    assert zr.shape == (20, 15 + 2 * G)
    j, li = 7, 4
    f = c2 - G + li
    acc = 0.0
    for i in range(T):
        acc = acc + x[j * T + i] * E[(f * (j * T + i)) % (2 * L), 0]
    assert zr[j, li] == acc
    P = tc.window_energies(zr, zi)
    assert P.shape == (13, 15 + 2 * G)
    re = ((zr[2, li] + zr[3, li]) + (zr[4, li] + zr[5, li])) + ((zr[6, li] + zr[7, li]) + (zr[8, li] + zr[9, li]))
    im = ((zi[2, li] + zi[3, li]) + (zi[4, li] + zi[5, li])) + ((zi[6, li] + zi[7, li]) + (zi[8, li] + zi[9, li]))
    assert P[2, li] == re * re + im * im
    y = rng.standard_normal(3 * L)
    Y = tc.symbols(y, 0, 1, baud, carrier, search=G)
    p = np.zeros(4)
    for i in range(L):
        p[i & 3] = p[i & 3] + y[L + i] * E[((c2 + 1 + 2 * 5) * i) % (2 * L), 1]
    assert Y[1, 5].imag == (p[0] + p[1]) + (p[2] + p[3])


def test_entry_argument_checks(product):
    import _amr
    import modem
    L = product
    inv = _amr.AMR_E_INVALID
    p = _amr.ptr
    x = np.zeros((1, 400), np.float32)
    out = np.zeros((1, 64), np.uint8)
    ln, sy, st, sh = (np.zeros(1, np.int64) for _ in range(4))
    soft = np.zeros((1, 512), np.int8)
    score = np.zeros(1)
    Y = np.zeros((1, 5, 8, 2))
    words = np.zeros((1, 1), np.uint32)
    assert L.amr_tone8_demod_host(None, p(x), 0, 1, 400, p(out), 64, p(ln), p(sy), p(soft), 512, p(st), p(sh), 1) == inv
    assert b"amr_tone8_demod_host" in L.amr_last_error()
    assert L.amr_tone8_demod_device(None, p(x), 0, 1, 400, p(out), 64, p(ln), p(sy), None, 0, None, None, 0) == inv
    assert L.amr_tone8_demod_host(None, p(x), 0, -1, 400, p(out), 64, p(ln), p(sy), None, 0, None, None, 1) == inv
    assert b"negative" in L.amr_last_error()
    assert L.amr_tone8_acquire_host(None, p(x), 0, 1, 400, p(st), p(sh), p(score)) == inv
    assert b"amr_tone8_acquire_host" in L.amr_last_error()
    assert L.amr_tone8_acquire_device(None, p(x), 0, 1, 400, p(st), p(sh), None) == inv
    assert L.amr_tone8_symbols_at_host(None, p(x), 0, 1, 400, p(st), p(sh), p(Y)) == inv
    assert L.amr_tone8_slice_host(p(Y), 1, 5, None) == inv and L.amr_tone8_slice_host(None, 1, 5, p(words)) == inv
    assert L.amr_tone8_soft_host(p(Y), 1, 5, None) == inv and L.amr_tone8_soft_host(p(Y), -1, 5, p(soft)) == inv
    assert L.amr_tone8_slice_host(None, 0, 0, None) == _amr.AMR_OK and L.amr_tone8_soft_host(p(Y), 1, 0, p(soft)) == _amr.AMR_OK
    assert L.amr_tone8_plan_out_capacity(None) == -1 and L.amr_tone8_plan_scratch_bytes(None) == -1
    assert L.amr_tone8_plan_synchronize(None) == inv and L.amr_tone8_plan_enable_timing(None, 1) == inv
    assert L.amr_tone8_plan_timings(None, None, 5) == inv and L.amr_tone8_plan_destroy(None) == _amr.AMR_OK
    # the score stage's checks
    P = np.zeros((1, 60, 21))
    peak = L.amr_tone8_peak_host
    assert peak(10, 3, None, 1, 60, p(st), p(sh), p(score)) == inv
    assert peak(10, 3, p(P), 1, 60, None, p(sh), p(score)) == inv
    assert peak(10, 3, p(P), 1, 60, p(st), None, p(score)) == inv
    assert peak(0, 3, p(P), 1, 60, p(st), p(sh), p(score)) == inv
    assert peak(10, 17, p(P), 1, 60, p(st), p(sh), p(score)) == inv
    assert peak(10, 3, p(P), -1, 60, p(st), p(sh), p(score)) == inv
    assert peak(10, 3, p(P), 1, -1, p(st), p(sh), p(score)) == inv
    assert peak(10, 3, None, 0, 60, None, None, None) == _amr.AMR_OK
    # the kernel's chunk: 64 start slots at the default search, fewer lines give more
    assert L.amr_tone8_chunk(6) == 64 == _amr.tone8_chunk() and L.amr_tone8_chunk(0) == 159 and L.amr_tone8_chunk(16) == 13
    assert L.amr_tone8_chunk(3) == 98 and L.amr_tone8_chunk(1) == 134 and L.amr_tone8_chunk(17) < 0 and L.amr_tone8_chunk(-1) < 0
    assert all((_amr.tone8_chunk(g) + 55) * (15 + 2 * g) <= 119 * 27 for g in range(17))
    # the modulator's checks
    Sn = _amr.design_tone8(1200, 3000.0, 96000, 0)[4]
    nb = np.array([3], np.int64)
    data = np.zeros((1, 3), np.uint8)
    o32 = np.zeros((1, 100), np.float32)
    mod = L.amr_tone8_modulate_host
    assert mod(80, 5, p(Sn), p(data), 3, p(nb), 1, p(o32), 99, 100, None, 0) == inv     # out_stride < n_out
    assert mod(80, 5, None, p(data), 3, p(nb), 1, p(o32), 100, 100, None, 0) == inv
    assert mod(80, 1, p(Sn), p(data), 3, p(nb), 1, p(o32), 100, 100, None, 0) == inv
    assert mod(80, 66, p(Sn), p(data), 3, p(nb), 1, p(o32), 100, 100, None, 0) == inv
    assert mod(84, 5, p(Sn), p(data), 3, p(nb), 1, p(o32), 100, 100, None, 0) == inv
    assert mod(80, 5, p(Sn), p(data), 2, p(nb), 1, p(o32), 100, 100, None, 0) == inv    # n_bytes > stride
    assert mod(80, 5, p(Sn), None, 0, None, 0, None, 0, 0, None, 0) == _amr.AMR_OK       # empty batch
    # the byte estimates are host arithmetic
    est, acq = L.amr_tone8_plan_bytes_estimate, L.amr_tone8_acquire_bytes_estimate
    nj = 96000 // 10 - 55
    assert acq(96000, 80, 6, 1) == -(-nj // 64) * 32 + 3 * 8                 # the chunks' maxima, start, shift, score
    assert acq(96000, 80, 3, 1) == -(-nj // 98) * 32 + 3 * 8
    assert acq(0, 80, 6, 2) == 32 + 2 * 3 * 8                                # no chunk
    assert acq(96000, 84, 6, 1) < 0 and acq(96000, 80, 6, 0) < 0 and acq(-1, 80, 6, 1) < 0 and acq(96000, 80, 17, 1) < 0
    e1, e2 = est(96000, 80, 6, 1), est(96000, 80, 6, 64)
    assert 0 < e1 < e2 < 64 * e1 + 1 and est(96000, 16, 6, 1) < 0 and est(96000, 80, 6, 0) < 0
    if _amr.device_count() < 1:
        z = np.zeros(4000, np.float32)
        for call in (lambda: modem.tone8_acquire(z, 1200, 3000.0, search=3),
                     lambda: modem.tone8_demodulate(z, 1200, 3000.0, search=3),
                     lambda: modem.tone8_demodulate_soft(z, 1200, 3000.0, acquire=False),
                     lambda: modem.tone8_modulate(b"FBPC", 1200, 3000.0),
                     lambda: modem.modulate_batch("tone8", [b"a"], 1200, 3000.0),
                     lambda: _amr.tone8_slice(np.ones((1, 3, 8), np.complex128)),
                     lambda: _amr.tone8_soft(np.ones((1, 3, 8), np.complex128)),
                     lambda: _amr.tone8_peak(np.ones((1, 60, 21)), 10, 3)):
            with pytest.raises(_amr.AmrError):
                call()
    with pytest.raises(ValueError):
        modem.tone8_acquire(np.zeros((2, 4000), np.float32), 1200, 3000.0, search=3)
    with pytest.raises(ValueError):
        modem.tone8_demodulate(np.zeros((2, 4000), np.float32), 1200, 3000.0, search=3)
    with pytest.raises(ValueError):
        modem.tone8_demodulate(np.zeros(4000, np.float32), 1200, 3000.0)     # the default search of 6 needs c2 >= 8
    with pytest.raises(ValueError):
        _amr.tone8_peak(np.ones((1, 60, 20)), 10, 3)
    empty = modem.tone8_acquire_batch(np.zeros((0, 100), np.float32), 1200, 3000.0, search=3)
    assert empty[0].shape == empty[1].shape == (0,)
    assert modem.tone8_demodulate_batch(np.zeros((0, 100), np.float32), 1200, 3000.0, search=3) == []
    assert modem.tone8_demodulate_soft_batch(np.zeros((0, 100), np.float32), 1200, 3000.0, search=3) == ([], [])


def test_the_aliases_are_untouched(product):
    """ft8_modulate / ft8_demodulate stay the reference's two-tone FSK calls at 50 Bd: nothing tone8."""
    import inspect
    import modem
    for fn in (modem.ft8_modulate, modem.ft8_demodulate):
        src = inspect.getsource(fn)
        assert "fsk_" in src and "50" in src and "tone8" not in src
