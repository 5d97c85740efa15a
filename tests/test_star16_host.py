"""The star16 definitions of DESIGN §3o without a GPU: the numpy restatement in
tests/star16_cases.py (the checker of the GPU kernels) decodes what it sends,
does not care about the capture's gain, its nibble map, ring rule, soft signs
and magnitudes hold what the design states, and the C ABI and Python surface
know the new kind and mode (argument checks only: no device work happens
before them)."""
import numpy as np
import pytest

import psk8_cases as p8
import star16_cases as s16

TAIL = 4                     # symbols of silence after the frame (see test_round_trip)


@pytest.fixture(scope="module")
def product(built_lib):
    """The restatement is only worth testing beside the product it restates."""
    import _amr
    import modem
    assert _amr.PSK_STAR16 == 4 and _amr.psk_kind("star16") == 4 and _amr.psk_bits("star16") == 4
    assert [_amr.psk_kind(k) for k in ("qpsk", "bpsk", "d8psk")] == [0, 1, 2]
    assert [_amr.psk_bits(k) for k in ("qpsk", "bpsk", "d8psk")] == [2, 1, 3]
    assert _amr.TX_MODES["star16"] == _amr.TX_STAR16 == 6
    for name in ("star16_modulate", "star16_demodulate", "star16_demodulate_batch", "star16_demodulate_soft",
                 "star16_demodulate_soft_batch"):
        assert callable(getattr(modem, name)), name
    return _amr.lib()


def payload(rng, n):
    return b"FBPC" + rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def capture(msg, baud, carrier):
    """The frame and TAIL symbols of silence after it."""
    x = s16.modulate(msg, baud, carrier)
    assert x.dtype == np.float32 and x.size == (40 + 2 * len(msg)) * int(96000 / baud)
    return np.concatenate([x, np.zeros(TAIL * int(96000 / baud), np.float32)])


def wrong_bits(data, msg):
    assert len(data) >= len(msg)
    return int(np.unpackbits(np.frombuffer(data[:len(msg)], np.uint8) ^ np.frombuffer(msg, np.uint8)).sum())


@pytest.mark.parametrize("sigma", [0.0, 0.02, 0.05])
@pytest.mark.parametrize("baud,carrier", s16.CONFIGS)
def test_round_trip(product, baud, carrier, sigma):
    """The restatement's demodulator recovers its modulator's payload after the sync: exactly when clean and,
    at the first four configurations, under N(0, 0.02^2); with at most 1 % of the payload bits wrong under
    N(0, 0.05^2) (a condition, not a measurement: the seeds are fixed).

    The capture runs TAIL symbols past the frame.  One that ends with the frame's last sample puts the last
    symbols inside filtfilt's odd extension, where the parabolic envelope has no flat top to mirror: over 60
    seeded frames per configuration the last three symbols then held 10, 7 and 6 wrong bits of 76 984 at
    2400 / 3000, 9600 / 12000 and 19200 / 24000 (none at the other two), and none anywhere with the tail
    (DESIGN §3o)."""
    rng = np.random.default_rng(int(baud) + int(sigma * 100))
    msg = payload(rng, int(rng.integers(60, 201)))
    x = capture(msg, baud, carrier)
    if sigma:
        x = x + rng.normal(0.0, sigma, x.size).astype(np.float32)
    data, sync = s16.demod(x, baud, carrier)
    # the first product is symbol 1's step: the sync follows the preamble's other 39 nibbles
    assert sync == 156
    bad = wrong_bits(data, msg)
    print(f"star16 round trip {baud}/{carrier} sigma {sigma}: {bad} wrong bits of {8 * len(msg)}")
    if sigma == 0.0 or (sigma == 0.02 and (baud, carrier) != s16.CONFIGS[4]):
        assert data[:len(msg)] == msg
    else:
        assert bad <= 0.01 * 8 * len(msg)
    sdata, soft, ssync = s16.demod_soft(x, baud, carrier)
    assert (sdata, ssync) == (data, sync) and np.packbits(soft > 0).tobytes() == data


@pytest.mark.parametrize("baud,carrier", [s16.CONFIGS[0], s16.CONFIGS[3], s16.CONFIGS[4]])
def test_gain_invariance(product, baud, carrier):
    """Every stage is linear and both decisions compare like with like: a power-of-two gain changes no bit.
    So does a float32 capture quantised to int16 at half scale against its own float64 image."""
    rng = np.random.default_rng(int(baud) + 16)
    msg = payload(rng, int(rng.integers(60, 201)))
    x = capture(msg, baud, carrier).astype(np.float64) + rng.normal(0.0, 0.05, (40 + 2 * len(msg) + TAIL) * (96000 // baud))
    want = s16.slice_bits(s16.symbols(x, baud, carrier))
    assert want.size == 4 * (40 + 2 * len(msg) + TAIL - 1)
    for g in (-40, -20, 20, 40):
        assert np.array_equal(s16.slice_bits(s16.symbols(np.ldexp(x, g), baud, carrier)), want), g
    q = np.round(np.clip(x, -1.9, 1.9) * 16384).astype(np.int16)
    bits_q = s16.slice_bits(s16.symbols(q.astype(np.float64), baud, carrier))
    assert np.array_equal(bits_q, s16.slice_bits(s16.symbols(q / 32768.0, baud, carrier)))
    assert s16.demod(q.astype(np.float64), baud, carrier)[0][:4] == b"FBPC"


def test_preamble_and_nibble_map(product):
    pre = np.packbits(s16.tx_bits(b"")).tobytes()
    assert pre == bytes(15) + bytes([0xEE]) * 5
    for n in (0, 1, 2, 3, 97):
        assert s16.tx_bits(bytes([0xFF]) * n).size == 160 + 8 * n
    ph, amp = s16.phases_amps(b"")
    assert ph.size == 40 and not ph[:30].any() and np.array_equal(ph[30:], np.pi * np.arange(1, 11))
    assert np.all(amp[:30] == 1.0) and amp[30:].tolist() == [0.5, 1.0] * 5       # the preamble visits both rings
    # one byte is two symbols, high nibble first: (a, b2, b1, b0), the tribit d8psk's
    ph, amp = s16.phases_amps(bytes([0x9C]))                                   # 1001 | 1100
    assert amp[40:].tolist() == [0.5, 1.0]
    steps = [p8.STEP[p8.INV_GRAY[1]], p8.STEP[p8.INV_GRAY[4]]]
    assert np.array_equal(ph[40:], [ph[39] + steps[0] * (np.pi / 4), ph[39] + steps[0] * (np.pi / 4) + steps[1] * (np.pi / 4)])
    # every nibble decides itself: symbol pairs with step m and every ring pair
    for m in range(8):
        for r0, r1 in ((1.0, 1.0), (1.0, 0.5), (0.5, 1.0), (0.5, 0.5)):
            sym = np.array([r0, r1 * np.exp(1j * np.pi / 4 * m)])
            want = [int(r0 != r1)] + [(int(p8.GRAY[m]) >> s) & 1 for s in (2, 1, 0)]
            assert s16.slice_bits(sym).tolist() == want, (m, r0, r1)
    env = s16.envelope(5)
    assert env.tolist() == [4.0 * (u * (1.0 - u)) for u in [(i + 0.5) / 5 for i in range(5)]]
    assert env[2] == 1.0 and np.allclose(env, [0.36, 0.84, 1.0, 0.84, 0.36], rtol=1e-15) and s16.envelope(1).tolist() == [1.0]


def test_ring_rule_is_total(product):
    nan, inf, tiny = np.nan, np.inf, 5e-324
    pairs = [(0.0, 0.0), (0.0, tiny), (tiny, 0.0), (nan, 1.0), (1.0, nan), (nan, nan), (inf, inf), (inf, 1.0),
             (1.0, inf), (1.0, 2.0), (2.0, 1.0), (1.0, np.nextafter(2.0, 3.0)), (np.nextafter(2.0, 3.0), 1.0),
             (1.0, np.nextafter(2.0, 1.0)), (3.0, 3.0), (0.0, 1.0), (1e308, 1e308), (1e308, 4e307)]
    want = [0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 0, 1]              # 2.0 * 1e308 overflows: neither compare holds
    got = [int(s16.ring_bits(np.array(p))[0]) for p in pairs]
    assert got == want
    # the soft value of a: 64 at equal energies, 51 at a clean ring change (energy ratio 4), 1 on the tie and on NaN
    e = np.array([1.0, 1.0, 4.0, 1.0, 2.0, nan, inf, inf])
    assert s16.ring_soft(e).tolist() == [-64, 51, 51, -1, -1, -1, -1]


def test_soft_signs_agree_with_the_hard_bits(product):
    """On 200 000 random symbol pairs of every scale the sign of (e1 > 2 e0) | (e0 > 2 e1) is the hard a, and all
    four soft signs are the hard nibble."""
    import soft_cases as sc
    rng = np.random.default_rng(16)
    n = 200000
    sym = rng.standard_normal(2 * n) + 1j * rng.standard_normal(2 * n)
    sym *= np.exp(rng.uniform(-40, 40, 2 * n))                                    # every scale, every ratio
    sym[: n // 2] = (sym[: n // 2] / np.abs(sym[: n // 2])) * rng.choice([0.5, 1.0], n // 2) * \
        (1 + 0.2 * rng.standard_normal(n // 2))                                  # and the two rings, noisy
    e = s16.energies(sym)
    nib = s16.nibbles(sym)
    assert nib.size == 2 * n - 1 and 0.1 < np.mean(nib >> 3) < 0.97
    assert np.array_equal(nib >> 3, ((e[1:] > 2.0 * e[:-1]) | (e[:-1] > 2.0 * e[1:])).astype(np.int64))
    assert np.array_equal(nib & 7, p8.tribits(sc.diff_products(sym)))
    s = s16.soft(sym)
    assert s.dtype == np.int8 and s.size == 4 * nib.size and not np.any(s == 0) and not np.any(s == -128)
    assert np.array_equal((s.reshape(-1, 4) > 0).astype(np.int64), (nib[:, None] >> np.array([3, 2, 1, 0])) & 1)
    assert np.array_equal(s.reshape(-1, 4)[:, 1:].ravel(), p8.soft_of_products(sc.diff_products(sym)))
    a = np.abs(s[0::4].astype(np.int64))
    assert a.max() == 127 and 60 <= a[(nib >> 3) == 0].max() <= 64                # no ring change: at most the equal-energy 64


# ---- the ABI's argument checks (no device work before them) ------------------
def test_plan_entries_know_the_kind(product):
    import _amr
    L = product
    d = L.amr_psk_plan_bytes_estimate(_amr.PSK_D8PSK, 96000, 5, 2, 9, 5, 64)
    s = L.amr_psk_plan_bytes_estimate(_amr.PSK_STAR16, 96000, 5, 2, 9, 5, 64)
    assert 0 < d < s                                         # 4 bits per symbol: more words, a longer output
    assert L.amr_psk_plan_bytes_estimate(3, 96000, 5, 2, 9, 5, 64) < 0
    assert L.amr_psk_plan_bytes_estimate(5, 96000, 5, 2, 9, 5, 64) < 0
    h = _amr.ctypes.c_void_p()
    z = np.zeros(16)
    for kind in (3, 5):
        assert L.amr_psk_plan_create(_amr.ctypes.byref(h), 0, kind, 96000, 5, 2, _amr.ptr(z), _amr.ptr(z), _amr.ptr(z),
                                     9, _amr.ptr(z), _amr.ptr(z), _amr.ptr(z), 5, _amr.ptr(z), 1) == _amr.AMR_E_INVALID
        assert b"unknown PSK kind" in L.amr_last_error() and not h.value
    # the kind is accepted: the next check (sps) is the one that refuses
    assert L.amr_psk_plan_create(_amr.ctypes.byref(h), 0, 4, 96000, 0, 2, _amr.ptr(z), _amr.ptr(z), _amr.ptr(z), 9,
                                 _amr.ptr(z), _amr.ptr(z), _amr.ptr(z), 5, _amr.ptr(z), 1) == _amr.AMR_E_INVALID
    assert b"sps" in L.amr_last_error()
    a, b = _amr.design_psk("star16", 4096, 9600, 12000.0), _amr.design_psk("qpsk", 4096, 9600, 12000.0)
    assert a[:2] == b[:2] and all(np.array_equal(u, v) for u, v in zip(a[2] + a[3], b[2] + b[3]))
    with pytest.raises(KeyError):
        _amr.design_psk("apsk16", 4096, 9600)
    with pytest.raises(KeyError):
        _amr.psk_bits("apsk16")


def test_symbol_stage_entries_know_the_kind(product):
    import _amr
    L = product
    sym = np.zeros((2, 4, 2))
    soft = np.zeros((2, 12), np.int8)
    words = np.zeros((2, 1), np.uint32)
    p = _amr.ptr
    for fn, out in ((L.amr_psk_soft_host, soft), (L.amr_psk_slice_host, words)):
        assert fn(5, p(sym), 2, 4, p(out)) == _amr.AMR_E_INVALID and b"unknown PSK kind" in L.amr_last_error()
        assert fn(4, p(sym), -1, 4, p(out)) == _amr.AMR_E_INVALID and b"unknown PSK kind" not in L.amr_last_error()
        assert fn(4, None, 2, 4, p(out)) == _amr.AMR_E_INVALID
        assert fn(4, p(sym), 2, 4, None) == _amr.AMR_E_INVALID
        assert fn(4, None, 0, 4, None) == _amr.AMR_OK          # an empty batch
        assert fn(4, p(sym), 2, 1, p(out)) == _amr.AMR_OK      # one symbol: no product, nothing written
    assert not soft.any() and not words.any()


def test_transmit_entries_know_the_mode(product):
    import _amr
    L = product
    for baud, nb in ((1200, 0), (1200, 1), (9600, 2), (19200, 3), (19200, 97), (96000, 5)):
        sps = int(96000 / baud)
        want = (40 + 2 * nb) * sps
        assert L.amr_tx_samples(_amr.TX_STAR16, nb, float(baud), 96000.0) == want
        assert _amr.tx_samples(_amr.TX_STAR16, nb, baud, 96000) == s16.modulate(bytes(nb), baud).size == want
        # the tables and, per stream and symbol, a phase and a ring amplitude
        assert L.amr_tx_work_bytes(_amr.TX_STAR16, float(baud), 96000.0, 3, want) >= (3 * sps + 2 * 3 * (want // sps)) * 8
        assert L.amr_tx_work_bytes(_amr.TX_STAR16, float(baud), 96000.0, 3, want) > \
            L.amr_tx_work_bytes(_amr.TX_D8PSK, float(baud), 96000.0, 3, want)
    assert L.amr_tx_samples(5, 1, 1200.0, 96000.0) == _amr.AMR_E_INVALID
    assert L.amr_tx_samples(7, 1, 1200.0, 96000.0) == _amr.AMR_E_INVALID
    assert L.amr_tx_samples(_amr.TX_STAR16, -1, 1200.0, 96000.0) == _amr.AMR_E_INVALID
    # fewer than one sample per symbol, refused before any device work
    assert L.amr_tx_samples(_amr.TX_STAR16, 1, 200000.0, 96000.0) == _amr.AMR_E_INVALID
    assert b"star16" in L.amr_last_error()
    assert L.amr_tx_work_bytes(_amr.TX_STAR16, 200000.0, 96000.0, 1, 10) == _amr.AMR_E_INVALID
    with pytest.raises(ValueError, match="star16"):
        s16.modulate(b"abc", 200000)
    data = np.zeros((1, 4), np.uint8)
    nbytes = np.array([4], np.int64)
    out = np.zeros((1, 16), np.float32)
    p = _amr.ptr
    assert L.amr_modulate_host(_amr.TX_STAR16, 200000.0, 3000.0, 0.0, 96000.0, p(data), 4, p(nbytes), 1, p(out), 16,
                               16, None, 0) == _amr.AMR_E_INVALID
    assert b"star16" in L.amr_last_error()
    assert L.amr_modulate_device(None, _amr.TX_STAR16, 200000.0, 3000.0, 0.0, 96000.0, p(data), 4, p(nbytes), 1,
                                 p(out), 16, 16, None, 0, None, 0) == _amr.AMR_E_INVALID
    assert not out.any()
