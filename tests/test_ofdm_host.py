"""The ofdm definitions of DESIGN §3j without a GPU: the numpy restatement in
tests/ofdm_cases.py (the checker of the GPU kernels) decodes what it sends,
also from a capture that starts late; its geometry refuses what the design
refuses; the decision rule is total and the soft signs are its bits; and the
C ABI refuses bad arguments before any device work."""
import ctypes

import numpy as np
import pytest

import ofdm_cases as oc

NOISE = [0.0, 0.05]
KS = [1, 3, 4, 8]


@pytest.fixture(scope="module")
def product(built_lib):
    """The restatement is only worth testing beside the product it restates."""
    import _amr
    import modem
    for name in ("ofdm_modulate", "ofdm_demodulate", "ofdm_demodulate_batch", "ofdm_demodulate_soft",
                 "ofdm_demodulate_soft_batch"):
        assert callable(getattr(modem, name)), name
    assert _amr.TO_NAMES == ["dft", "slice", "sync_pack", "launch"]
    return _amr.lib()


def payload(rng, n):
    return b"FBPC" + rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def check_decoded(data, sync, msg, K):
    """The payload exactly after the sync, then only the zero padding to a multiple of 2 K bits."""
    total = oc.tx_bits(msg, K).size
    assert sync == oc.SYNC_AT
    assert len(data) == (total - oc.SYNC_AT) // 8 and data[:len(msg)] == msg and not any(data[len(msg):])


@pytest.mark.parametrize("sigma", NOISE)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("baud,carrier", oc.CONFIGS)
def test_round_trip(product, baud, carrier, K, sigma):
    assert oc.valid(baud, carrier, K)                        # all twenty are (checked when the cases were chosen)
    rng = np.random.default_rng(int(baud) + 100 * K + int(sigma * 100))
    msg = payload(rng, int(rng.integers(60, 201)))
    x = oc.modulate(msg, baud, carrier, K)
    sps, L, Ncp, Nu, bins = oc.geometry(baud, carrier, K)
    assert x.dtype == np.float32 and x.size == oc.n_symbols(len(msg), K) * L and L == K * sps and Ncp + Nu == L
    assert np.abs(x).max() <= 1.0
    if sigma:
        x = x + rng.normal(0.0, sigma, x.size).astype(np.float32)
    data, sync = oc.demod(x, baud, carrier, K)
    check_decoded(data, sync, msg, K)
    sdata, soft, ssync = oc.demod_soft(x, baud, carrier, K)
    assert (sdata, ssync) == (data, sync) and np.packbits(soft > 0).tobytes() == data


@pytest.mark.parametrize("K", [16, 64])
def test_round_trip_many_subcarriers_clean(product, K):
    """Amplitude is 1 / K per subcarrier: K = 16 and 64 are pinned clean only."""
    rng = np.random.default_rng(K)
    msg = payload(rng, 150)
    data, sync = oc.demod(oc.modulate(msg, 9600, 12000.0, K), 9600, 12000.0, K)
    check_decoded(data, sync, msg, K)


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("late", ["one", "Ncp"])
def test_late_start_decodes_the_same(product, K, late):
    """The decision is differential in time per subcarrier: d <= Ncp zero samples
    in front rotate every subcarrier by a constant and change no byte."""
    baud, carrier = 9600, 12000.0
    rng = np.random.default_rng(5 + K)
    msg = payload(rng, 90)
    x = oc.modulate(msg, baud, carrier, K)
    Ncp = oc.geometry(baud, carrier, K)[2]
    assert Ncp >= 1
    d = 1 if late == "one" else Ncp
    want = oc.demod(x, baud, carrier, K)
    got = oc.demod(np.concatenate([np.zeros(d, np.float32), x]), baud, carrier, K)
    assert got == want
    check_decoded(*got, msg, K)


def test_preamble_padding_and_phases(product):
    assert np.packbits(oc.tx_bits(b"", 4)).tobytes() == bytes(7) + bytes([0x0F, 0xFF, 0xFF])
    for K in (1, 3, 8, 64):
        for n in (0, 1, 5):
            bits = oc.tx_bits(bytes([0xFF]) * n, K)
            assert bits.size % (2 * K) == 0 and bits.size - (80 + 8 * n) < 2 * K and not bits[80 + 8 * n:].any()
            assert oc.phases(bytes(n), K).shape == (oc.n_symbols(n, K), K)
    ph = oc.phases(b"\x1b", 4)                               # dibits 00 01 10 11 on symbol 11
    assert np.array_equal(ph[0], np.pi * np.array([0, 1, 4, 9]) / 4)
    assert np.array_equal(ph[7], ph[0]) and np.array_equal(ph[8], ph[0] + np.array([0, 0, np.pi, np.pi]))
    assert np.array_equal(ph[11] - ph[10], (ph[10] + oc.STEPS) - ph[10])


def test_invalid_geometry(product):
    import _amr
    import modem
    L = product
    bad = [(9600, 12000.0, 0), (9600, 12000.0, 65),          # K outside 1..64
           (1200, 100.0, 8),                                 # bins[0] = 1 - 4 < 1
           (9600, 45000.0, 8),                               # 2 * bins[7] = 72 >= Nu = 70
           (200000, 12000.0, 4)]                             # sps = 0
    x = np.zeros(4000, np.float32)
    for baud, carrier, K in bad:
        assert not oc.valid(baud, carrier, K)
        with pytest.raises(ValueError):
            _amr.design_ofdm(baud, carrier, K)
        with pytest.raises(ValueError):
            modem.ofdm_modulate(b"abc", baud, carrier, K)
        with pytest.raises(ValueError):
            modem.ofdm_demodulate(x, baud, carrier, K)
        with pytest.raises(ValueError):
            modem.ofdm_demodulate_soft_batch(x[None, :], baud, carrier, K)
        with pytest.raises(ValueError):
            modem.modulate_batch("ofdm", [b"abc"], baud, carrier, num_subcarriers=K)
        # the C layer, before any device work
        data = np.zeros((1, 4), np.uint8)
        nb = np.array([3], np.int64)
        out = np.full((1, 64), 7.0, np.float32)
        assert L.amr_ofdm_modulate_host(float(baud), float(carrier), 96000.0, K, _amr.ptr(data), 4, _amr.ptr(nb), 1,
                                        _amr.ptr(out), 64, 64, None, 0) == _amr.AMR_E_INVALID
        assert b"ofdm" in L.amr_last_error() and (out == 7.0).all()
    # the edges that are valid: bins[0] == 1, and 2 * bins[K-1] == Nu - 2 (Nu even) or Nu - 1 (Nu odd)
    assert oc.geometry(9600, 6200.0, 8)[4][0] == 1                          # c0 = 5 at Nu = 70
    assert not oc.valid(9600, 6100.0, 8)                                    # c0 = 4: bins[0] = 0
    assert oc.geometry(9600, 42515.0, 8)[4][-1] == 34                       # c0 = 31: 2 * 34 = 68 < 70
    assert not oc.valid(9600, 43886.0, 8)                                   # c0 = 32: 2 * 35 = 70
    with pytest.raises(ValueError):
        modem.modulate_batch("ofdm", [b"abc"], 9600, 12000.0)               # num_subcarriers is required


def test_plan_create_argument_checks(product):
    import _amr
    L = product
    h = ctypes.c_void_p()
    sps, Lsym, Ncp, Nu, bins, W = _amr.design_ofdm(9600, 12000.0, 8)
    create = L.amr_ofdm_plan_create
    ref = ctypes.byref(h)
    b, w = _amr.ptr(bins), _amr.ptr(W)
    inv = _amr.AMR_E_INVALID
    assert create(None, 0, 4000, sps, 8, b, w, 1) == inv
    assert create(ref, 0, 4000, sps, 8, None, w, 1) == inv
    assert create(ref, 0, 4000, sps, 8, b, None, 1) == inv
    assert create(ref, 0, 4000, sps, 8, b, w, 0) == inv
    assert create(ref, 0, -1, sps, 8, b, w, 1) == inv
    assert create(ref, 0, 4000, sps, 0, b, w, 1) == inv
    assert create(ref, 0, 4000, sps, 65, b, w, 1) == inv and b"1..64" in L.amr_last_error()
    assert create(ref, 0, 4000, 0, 8, b, w, 1) == inv and b"sample per dibit" in L.amr_last_error()
    low = (bins - bins[0]).astype(np.int32)                                  # bins[0] = 0
    assert create(ref, 0, 4000, sps, 8, _amr.ptr(low), w, 1) == inv and b"below bin 1" in L.amr_last_error()
    assert bins.tolist() == list(range(5, 13)) and Nu == 70
    high = (bins + 23).astype(np.int32)                                      # 2 * 35 >= 70
    assert create(ref, 0, 4000, sps, 8, _amr.ptr(high), w, 1) == inv and b"Nu / 2" in L.amr_last_error()
    gap = bins.copy()
    gap[3] += 1
    assert create(ref, 0, 4000, sps, 8, _amr.ptr(gap), w, 1) == inv and b"consecutive" in L.amr_last_error()
    assert not h.value
    # the byte estimate is host arithmetic: it grows with the streams and refuses what create refuses
    est = [L.amr_ofdm_plan_bytes_estimate(96000, 10, 8, m) for m in (1, 64, 4096)]
    assert 0 < est[0] < est[1] < est[2]
    # per stream: x staged as float64, Y (1200 symbols x 8 x 16 B), words, bytes
    assert 96000 * 8 + 1200 * 128 < est[2] / 4096 < 96000 * 8 + 1200 * 128 + 8192
    assert L.amr_ofdm_plan_bytes_estimate(96000, 10, 65, 1) < 0
    assert L.amr_ofdm_plan_bytes_estimate(96000, 0, 8, 1) < 0
    assert L.amr_ofdm_plan_bytes_estimate(96000, 1, 8, 1) < 0                # Nu = 7: no bin below Nu / 2 with K = 8
    assert L.amr_ofdm_plan_bytes_estimate(96000, 10, 8, 0) < 0
    for fn in (L.amr_ofdm_plan_synchronize, L.amr_ofdm_plan_scratch_bytes, L.amr_ofdm_plan_out_capacity):
        assert fn(None) < 0
    assert L.amr_ofdm_plan_enable_timing(None, 1) == inv
    assert L.amr_ofdm_plan_timings(None, None, 4) == inv
    assert L.amr_ofdm_plan_destroy(None) == _amr.AMR_OK


def test_entry_argument_checks(product):
    import _amr
    L = product
    inv = _amr.AMR_E_INVALID
    x = np.zeros((1, 400), np.float32)
    out = np.zeros((1, 64), np.uint8)
    ln = np.zeros(1, np.int64)
    sy = np.zeros(1, np.int64)
    soft = np.zeros((1, 512), np.int8)
    Y = np.zeros((1, 4, 3, 2))
    p = _amr.ptr
    assert L.amr_ofdm_demod_host(None, p(x), 0, 1, 400, p(out), 64, p(ln), p(sy)) == inv
    assert L.amr_ofdm_demod_device(None, p(x), 0, 1, 400, p(out), 64, p(ln), p(sy)) == inv
    assert L.amr_ofdm_demod_soft_host(None, p(x), 0, 1, 400, p(out), 64, p(ln), p(sy), p(soft), 512) == inv
    assert L.amr_ofdm_demod_soft_device(None, p(x), 0, 1, 400, p(out), 64, p(ln), p(sy), p(soft), 512) == inv
    assert L.amr_ofdm_demod_soft_host(None, p(x), 0, -1, 400, p(out), 64, p(ln), p(sy), p(soft), 512) == inv
    assert L.amr_ofdm_symbols_host(None, p(x), 0, 1, 400, p(Y)) == inv
    words = np.zeros((1, 1), np.uint32)
    sv = np.zeros((1, 18), np.int8)
    for fn, o in ((L.amr_ofdm_slice_host, words), (L.amr_ofdm_soft_host, sv)):
        assert fn(p(Y), 1, 4, 0, p(o)) == inv and b"1..64" in L.amr_last_error()
        assert fn(p(Y), 1, 4, 65, p(o)) == inv
        assert fn(p(Y), -1, 4, 3, p(o)) == inv
        assert fn(None, 1, 4, 3, p(o)) == inv
        assert fn(p(Y), 1, 4, 3, None) == inv
        assert fn(None, 0, 4, 3, None) == _amr.AMR_OK            # an empty batch
        assert fn(p(Y), 1, 1, 3, p(o)) == _amr.AMR_OK            # one symbol: no product, nothing written
    assert not words.any() and not sv.any()
    data = np.zeros((1, 4), np.uint8)
    nb = np.array([4], np.int64)
    o = np.zeros((1, 64), np.float32)
    mod = L.amr_ofdm_modulate_host
    assert mod(9600.0, 12000.0, 96000.0, 8, p(data), 4, p(nb), -1, p(o), 64, 64, None, 0) == inv
    assert mod(9600.0, 12000.0, 96000.0, 8, p(data), 4, p(nb), 1, p(o), 32, 64, None, 0) == inv      # out_stride < n_out
    assert mod(9600.0, 12000.0, 96000.0, 8, p(data), 4, None, 1, p(o), 64, 64, None, 0) == inv
    assert mod(0.0, 12000.0, 96000.0, 8, p(data), 4, p(nb), 1, p(o), 64, 64, None, 0) == inv
    assert mod(float("nan"), 12000.0, 96000.0, 8, p(data), 4, p(nb), 1, p(o), 64, 64, None, 0) == inv
    nb[0] = 5                                                                                         # > data_stride
    assert mod(9600.0, 12000.0, 96000.0, 8, p(data), 4, p(nb), 1, p(o), 64, 64, None, 0) == inv
    assert mod(9600.0, 12000.0, 96000.0, 8, None, 0, None, 0, None, 0, 0, None, 0) == _amr.AMR_OK     # an empty batch
    assert not o.any()


def test_decision_rule_is_total(product):
    nan, inf = np.nan, np.inf
    d = np.array([0, -0.0, complex(nan, 1), complex(1, nan), complex(inf, inf), complex(-inf, inf), complex(inf, 1),
                  complex(1, -inf), 1 + 1j, -1 - 1j, 1 - 1j, -1 + 1j, -2 + 1j, 2 - 1j, complex(0, 5e-324)],
                 np.complex128)
    # zeros, a NaN component, inf against inf and exact ties compare false: the second line, by di's sign alone
    assert oc.sectors(d).tolist() == [3, 3, 1, 3, 1, 1, 0, 3, 1, 3, 3, 1, 2, 0, 1]
    assert oc.dibits(d).tolist() == [2, 2, 1, 2, 1, 1, 0, 2, 1, 2, 2, 1, 3, 0, 1]
    # the sector centres decide their own index, and the phase steps are those centres
    assert oc.sectors(np.exp(1j * np.pi / 2 * np.arange(4))).tolist() == [0, 1, 2, 3]
    assert np.allclose(np.exp(1j * oc.STEPS[oc.DIBIT]), np.exp(1j * np.pi / 2 * np.arange(4)))
    s = oc.soft_of_products(d)
    assert s.size == 2 * d.size and not np.any(s == 0) and not np.any(s == -128)
    assert np.array_equal((s.reshape(-1, 2) > 0).astype(np.int64), (oc.dibits(d)[:, None] >> np.array([1, 0])) & 1)


def test_soft_signs_agree_with_the_hard_bits(product):
    """Away from ties the two signed expressions' signs are the hard rule's bits, on 200 000 random products of every scale."""
    rng = np.random.default_rng(10)
    d = rng.standard_normal(200000) + 1j * rng.standard_normal(200000)
    d[:50000] *= np.exp(rng.uniform(-40, 40, 50000))         # every scale
    d[50000:60000] *= 2.0 ** rng.integers(-480, 480, 10000)
    dr, di = d.real, d.imag
    g = oc.dibits(d)
    assert np.array_equal((g >> 1) & 1, (dr + di < 0).astype(np.int64))      # hi bit: below the anti-diagonal
    assert np.array_equal(g & 1, (dr - di < 0).astype(np.int64))             # lo bit: above the diagonal
    s = oc.soft_of_products(d)
    assert s.dtype == np.int8 and s.size == 2 * d.size and not np.any(s == 0) and not np.any(s == -128)
    assert np.array_equal((s.reshape(-1, 2) > 0).astype(np.int64), (g[:, None] >> np.array([1, 0])) & 1)
    assert np.abs(s).max() == 127 and np.abs(s).min() == 1
    # by hand: on the real axis both bits are as far from their lines as they get
    assert oc.soft_of_products(np.array([1.0, -1.0, 1j, 3 + 1j])).tolist() == [-127, -127, 127, 127, -127, 127, -127, -64]
