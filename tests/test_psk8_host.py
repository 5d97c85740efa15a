"""The d8psk definitions of DESIGN §3i without a GPU: the numpy restatement in
tests/psk8_cases.py (the checker of the GPU kernels) decodes what it sends,
its Gray map, soft signs and magnitudes hold what the design states, and the
C ABI and Python surface know the new kind and mode (argument checks only:
no device work happens before them)."""
import numpy as np
import pytest

import psk8_cases as p8

NOISE = [0.0, 0.05]


@pytest.fixture(scope="module")
def product(built_lib):
    """The restatement is only worth testing beside the product it restates."""
    import _amr
    import modem
    assert _amr.PSK_KINDS == {"qpsk": 0, "bpsk": 1, "d8psk": 2} and _amr.PSK_D8PSK == 2
    assert _amr.PSK_BITS == {"qpsk": 2, "bpsk": 1, "d8psk": 3}
    assert _amr.TX_MODES["d8psk"] == _amr.TX_D8PSK == 4
    for name in ("d8psk_modulate", "d8psk_demodulate", "d8psk_demodulate_batch", "d8psk_demodulate_soft",
                 "d8psk_demodulate_soft_batch"):
        assert callable(getattr(modem, name)), name
    return _amr.lib()


def payload(rng, n):
    return b"FBPC" + rng.integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("sigma", NOISE)
@pytest.mark.parametrize("baud,carrier", p8.CONFIGS)
def test_round_trip(product, baud, carrier, sigma):
    """The restatement's demodulator recovers its modulator's payload exactly after the sync."""
    rng = np.random.default_rng(int(baud) + int(sigma * 100))
    msg = payload(rng, int(rng.integers(60, 201)))
    x = p8.modulate(msg, baud, carrier)
    assert x.dtype == np.float32 and x.size == (40 + -(-8 * len(msg) // 3)) * int(96000 / baud)
    if sigma:
        x = x + rng.normal(0.0, sigma, x.size).astype(np.float32)
    data, sync = p8.demod(x, baud, carrier)
    # the first product is symbol 1's step: the sync follows the preamble's other 39 tribits
    assert sync == 117 and data == msg
    sdata, soft, ssync = p8.demod_soft(x, baud, carrier)
    assert (sdata, ssync) == (data, sync) and np.packbits(soft > 0).tobytes() == data


def test_preamble_and_tail_padding(product):
    pre = np.packbits(p8.tx_bits(b"")).tobytes()
    assert pre == bytes(11) + bytes([0x36, 0xDB, 0x6D, 0xB6])
    for n, pad in ((0, 0), (1, 1), (2, 2), (3, 0), (4, 1)):
        bits = p8.tx_bits(bytes([0xFF]) * n)
        assert bits.size == 120 + 8 * n + pad and bits.size % 3 == 0 and not bits[120 + 8 * n:].any()
    ph = p8.phases(b"")
    assert ph.size == 40 and not ph[:30].any() and np.array_equal(ph[30:], np.pi * np.arange(1, 11))


def test_gray_neighbours_differ_in_one_bit(product):
    assert np.array_equal(p8.GRAY, np.arange(8) ^ (np.arange(8) >> 1))
    assert np.array_equal(p8.GRAY[p8.INV_GRAY], np.arange(8))
    for m in range(8):
        assert bin(int(p8.GRAY[m] ^ p8.GRAY[(m + 1) % 8])).count("1") == 1
    # the sector centres decide their own index, and the phase steps are those centres
    centres = np.exp(1j * np.pi / 4 * np.arange(8))
    assert p8.steps(centres).tolist() == list(range(8))
    assert np.allclose(np.exp(1j * np.pi / 4 * np.array(p8.STEP)), centres)


def test_decision_rule_is_total(product):
    nan, inf = np.nan, np.inf
    d = np.array([0, -0.0, complex(nan, 1), complex(1, nan), complex(inf, inf), complex(-inf, inf), complex(inf, 1),
                  complex(1, -inf), complex(1, p8.T), complex(5e-324, 0)], np.complex128)
    # zeros, a NaN component and inf / inf compare false on both axes: the last branch, by the signs alone;
    # so does the smallest denormal on the real axis (T * 5e-324 rounds to 0, and 0 < 0 is false)
    assert p8.steps(d).tolist() == [5, 5, 3, 7, 1, 3, 0, 6, 1, 7]


def test_soft_signs_agree_with_the_hard_bits(product):
    """The three signed expressions' signs are the hard rule's bits on 200 000 random products, and b0 stays <= 75."""
    rng = np.random.default_rng(8)
    d = rng.standard_normal(200000) + 1j * rng.standard_normal(200000)
    d[:50000] *= np.exp(rng.uniform(-40, 40, 50000))         # every scale
    dr, di = d.real, d.imag
    g = p8.tribits(d)
    e2 = di + p8.T * dr                                      # b2 = 1 iff below the line through 7pi/8, -pi/8
    e1 = p8.T * di - dr                                      # b1 = 1 iff left of the line through 3pi/8, -5pi/8
    a, b = di - p8.T * dr, dr + p8.T * di                    # b0: the pair through pi/8 and the pair through 5pi/8
    assert np.array_equal((g >> 2) & 1, (e2 < 0).astype(np.int64))
    assert np.array_equal((g >> 1) & 1, (e1 > 0).astype(np.int64))
    assert np.array_equal(g & 1, ((a > 0) != (b < 0)).astype(np.int64))
    s = p8.soft_of_products(d)
    assert s.dtype == np.int8 and s.size == 3 * d.size and not np.any(s == 0) and not np.any(s == -128)
    assert np.array_equal((s.reshape(-1, 3) > 0).astype(np.int64), (g[:, None] >> np.array([2, 1, 0])) & 1)
    assert np.abs(s[2::3]).max() <= 75 and np.abs(s[2::3]).max() >= 73
    assert np.abs(s[0::3]).max() == 127 and np.abs(s[1::3]).max() == 127


def test_soft_magnitudes_on_plain_values(product):
    """By hand: on the real axis b2 and b1 are far from their lines and b0 is at its maximum; on a sector
    boundary the bit that changes there is at its edge."""
    s = p8.soft_of_products(np.array([1.0, complex(1, p8.T), 0, complex(np.nan, 1)], np.complex128))
    # d = 1: den = 1, b2 = |T| -> 53, b1 = |-1| -> 127, b0 = min(|-T|, |1|) -> 53; tribit 000
    assert s[:3].tolist() == [-53, -127, -53]
    # d = 1 + T j, the pi/8 boundary (falls to sector 1, tribit 001): b0 at its edge
    assert s[3] < 0 and s[4] < 0 and s[5] == 1
    assert s[6:].tolist() == [1, 1, 1, -1, 1, -1]            # a zero: magnitude 1, tribit 111; NaN + 1j: step 3, tribit 010


# ---- the ABI's argument checks (no device work before them) ------------------
def test_plan_entries_know_the_kind(product):
    import _amr
    L = product
    q = L.amr_psk_plan_bytes_estimate(_amr.PSK_QPSK, 96000, 5, 2, 9, 5, 64)
    d = L.amr_psk_plan_bytes_estimate(_amr.PSK_D8PSK, 96000, 5, 2, 9, 5, 64)
    assert 0 < q < d                                         # 3 bits per symbol: more words, a longer output
    assert L.amr_psk_plan_bytes_estimate(3, 96000, 5, 2, 9, 5, 64) < 0
    h = _amr.ctypes.c_void_p()
    z = np.zeros(16)
    assert L.amr_psk_plan_create(_amr.ctypes.byref(h), 0, 3, 96000, 5, 2, _amr.ptr(z), _amr.ptr(z), _amr.ptr(z), 9,
                                 _amr.ptr(z), _amr.ptr(z), _amr.ptr(z), 5, _amr.ptr(z), 1) == _amr.AMR_E_INVALID
    assert b"unknown PSK kind" in L.amr_last_error() and not h.value
    # the kind is accepted: the next check (sps) is the one that refuses
    assert L.amr_psk_plan_create(_amr.ctypes.byref(h), 0, 2, 96000, 0, 2, _amr.ptr(z), _amr.ptr(z), _amr.ptr(z), 9,
                                 _amr.ptr(z), _amr.ptr(z), _amr.ptr(z), 5, _amr.ptr(z), 1) == _amr.AMR_E_INVALID
    assert b"sps" in L.amr_last_error()
    a, b = _amr.design_psk("d8psk", 4096, 9600, 12000.0), _amr.design_psk("qpsk", 4096, 9600, 12000.0)
    assert a[:2] == b[:2] and all(np.array_equal(u, v) for u, v in zip(a[2] + a[3], b[2] + b[3]))
    with pytest.raises(KeyError):
        _amr.design_psk("psk8", 4096, 9600)


def test_symbol_stage_entries_know_the_kind(product):
    import _amr
    L = product
    sym = np.zeros((2, 4, 2))
    soft = np.zeros((2, 9), np.int8)
    words = np.zeros((2, 1), np.uint32)
    p = _amr.ptr
    for fn, out in ((L.amr_psk_soft_host, soft), (L.amr_psk_slice_host, words)):
        assert fn(3, p(sym), 2, 4, p(out)) == _amr.AMR_E_INVALID and b"unknown PSK kind" in L.amr_last_error()
        assert fn(2, p(sym), -1, 4, p(out)) == _amr.AMR_E_INVALID
        assert fn(2, None, 2, 4, p(out)) == _amr.AMR_E_INVALID
        assert fn(2, p(sym), 2, 4, None) == _amr.AMR_E_INVALID
        assert fn(2, None, 0, 4, None) == _amr.AMR_OK          # an empty batch
        assert fn(2, p(sym), 2, 1, p(out)) == _amr.AMR_OK      # one symbol: no product, nothing written
    assert not soft.any() and not words.any()


def test_transmit_entries_know_the_mode(product):
    import _amr
    L = product
    for baud, nb in ((1200, 0), (1200, 1), (9600, 2), (19200, 3), (19200, 97), (96000, 5)):
        sps = int(96000 / baud)
        want = (40 + -(-8 * nb // 3)) * sps
        assert L.amr_tx_samples(_amr.TX_D8PSK, nb, float(baud), 96000.0) == want
        assert _amr.tx_samples(_amr.TX_D8PSK, nb, baud, 96000) == p8.modulate(bytes(nb), baud).size == want
        assert L.amr_tx_work_bytes(_amr.TX_D8PSK, float(baud), 96000.0, 3, want) >= (3 * sps + 3 * (want // sps)) * 8
    assert L.amr_tx_samples(5, 1, 1200.0, 96000.0) == _amr.AMR_E_INVALID
    assert L.amr_tx_samples(_amr.TX_D8PSK, -1, 1200.0, 96000.0) == _amr.AMR_E_INVALID
    # fewer than one sample per symbol, refused before any device work; QPSK's empty ramp stays its ValueError
    assert L.amr_tx_samples(_amr.TX_D8PSK, 1, 200000.0, 96000.0) == _amr.AMR_E_INVALID
    assert b"d8psk" in L.amr_last_error()
    assert L.amr_tx_work_bytes(_amr.TX_D8PSK, 200000.0, 96000.0, 1, 10) == _amr.AMR_E_INVALID
    assert L.amr_tx_samples(_amr.TX_QPSK, 1, 19200.0, 96000.0) == _amr.AMR_E_INVALID
    assert b"could not broadcast" in L.amr_last_error()
    data = np.zeros((1, 4), np.uint8)
    nbytes = np.array([4], np.int64)
    out = np.zeros((1, 16), np.float32)
    p = _amr.ptr
    assert L.amr_modulate_host(_amr.TX_D8PSK, 200000.0, 3000.0, 0.0, 96000.0, p(data), 4, p(nbytes), 1, p(out), 16, 16,
                               None, 0) == _amr.AMR_E_INVALID
    assert L.amr_modulate_device(None, _amr.TX_D8PSK, 200000.0, 3000.0, 0.0, 96000.0, p(data), 4, p(nbytes), 1, p(out),
                                 16, 16, None, 0, None, 0) == _amr.AMR_E_INVALID
    assert not out.any()
