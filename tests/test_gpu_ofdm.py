"""ofdm on the GPU: k_ofdm_dft, k_ofdm_slice, k_ofdm_soft and the
transmit kernels (ofdm_kernels.hip) with the plan / host layer around them,
against the numpy restatement in tests/ofdm_cases.py.  The receive side is
bit-equal to the restatement; the transmit samples are under
test_gpu_tx.assert_close's rule (sin's last ulp)."""
import numpy as np
import pytest

import ofdm_cases as oc
import soft_cases as sc
import viterbi_cases as vc
from test_gpu_tx import assert_close
from test_gpu_viterbi import Dev

pytestmark = pytest.mark.gpu

# (K, sps): Nu = 7, 29, 35, 35, 70, 140, 70, 168 -- Nu mod 4 = 3, 1, 3, 3, 2, 0, 2, 0; one chunk of the
# DFT kernel (Nu < 32), a chunk and a tail, several chunks; groups of 1, 3, 4, 4 + 1, 4 + 4, 4 x 4, 4 x 16 subcarriers
GEOS = [(1, 8), (3, 11), (4, 10), (5, 8), (8, 10), (8, 20), (16, 5), (64, 3)]
SYMBOLS = [0, 1, 2, 3, 63, 64, 65]
STREAMS = [1, 2, 65]


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")
    assert "amr_ofdm_plan_create" in _amr.EXPORTS            # the restatement is only worth testing beside the product


def cfg(K, sps):
    """(baud, carrier, K, samp_rate) with exactly sps samples per dibit and the subcarriers around fs / 4."""
    fs = 1000 * sps
    return 1000, fs / 4.0, K, fs


def same_bits(a, b):
    """Bit-equal float64 data; a NaN may differ in sign and payload (the host's default NaN is negative)."""
    a = np.ascontiguousarray(a).view(np.float64).ravel()
    b = np.ascontiguousarray(b).view(np.float64).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return a.size == b.size and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def want_Y(x, c):
    return np.stack([oc.symbols(r, *c) for r in x]) if len(x) else np.zeros((0, 0, c[2]), np.complex128)


def plan_for(n, c, B):
    import _amr
    baud, carrier, K, fs = c
    return _amr.OfdmPlan(n, baud, carrier, K, fs, max_streams=B)


# ---- 1. the DFT stage alone ---------------------------------------------------------------
def test_the_geometries_cover_what_they_should():
    nus = [oc.geometry(*cfg(K, sps))[3] for K, sps in GEOS]
    assert nus == [7, 29, 35, 35, 70, 140, 70, 168] and {nu % 4 for nu in nus} == {0, 1, 2, 3}
    assert {K for K, _ in GEOS} == {1, 3, 4, 5, 8, 16, 64}


@pytest.mark.parametrize("K,sps", GEOS)
def test_dft_geometries(K, sps):
    c = cfg(K, sps)
    L = K * sps
    rng = np.random.default_rng(100 * K + sps)
    x = rng.standard_normal((3, 5 * L + 1)).astype(np.float32)
    pl = plan_for(x.shape[1], c, 3)
    got = pl.symbols(x)
    assert got.shape == (3, 5, K) and same_bits(got, want_Y(x, c))
    assert np.abs(got).max() > 1.0                           # not the zeros of a kernel that did not run


@pytest.mark.parametrize("S", SYMBOLS)
@pytest.mark.parametrize("K,sps", [(8, 10), (3, 11)])
def test_dft_symbol_and_stream_counts(K, sps, S):
    """Flat symbol indices b*S + s cross wave and workgroup edges inside and between streams; a partial tail
    symbol of 0, 1 and L - 1 samples is ignored."""
    c = cfg(K, sps)
    L = K * sps
    rng = np.random.default_rng(1000 * K + S)
    for B, r in zip(STREAMS, (0, 1, L - 1)):
        n = S * L + r
        x = rng.standard_normal((B, n)).astype(np.float32)
        pl = plan_for(n, c, B)
        assert pl.S == S
        got = pl.symbols(x)
        assert got.shape == (B, S, K), (B, r)
        if S:
            assert same_bits(got, want_Y(x, c)), (B, r)
    # a plan larger than the batch, and a second call on it
    pl = plan_for(S * L + 2, c, 70)
    x = rng.standard_normal((3, S * L + 2))
    for _ in range(2):
        got = pl.symbols(x)
        assert got.shape == (3, S, K) and (S == 0 or same_bits(got, want_Y(x, c)))


@pytest.mark.parametrize("dt", ["f32", "f64", "i16"])
def test_dft_dtypes_and_row_stride(dt):
    c = cfg(8, 10)
    n = 7 * 80 + 5
    rng = np.random.default_rng(3)
    wide = rng.standard_normal((5, n + 13))
    wide = np.round(wide * 9000).astype(np.int16) if dt == "i16" else wide.astype({"f32": np.float32, "f64": np.float64}[dt])
    x = wide[:, :n]                                          # rows of a wider array: x_stride = n + 13
    assert x.strides[0] == (n + 13) * x.itemsize
    pl = plan_for(n, c, 8)
    assert same_bits(pl.symbols(x), want_Y(x, c))
    assert same_bits(pl.symbols(np.ascontiguousarray(x)), want_Y(x, c))


def test_dft_special_samples():
    """+-inf, NaN, denormals and all zeros: float64 arithmetic has one answer for each (a NaN's sign aside)."""
    c = cfg(8, 10)
    n = 4 * 80
    rng = np.random.default_rng(4)
    x = rng.standard_normal((8, n))
    x[0] = 0.0
    x[1] = -0.0
    x[2, 95] = np.inf
    x[3, 100] = -np.inf
    x[3, 101] = np.inf
    x[4, 200] = np.nan
    x[5] = 5e-324 * rng.integers(-3, 4, n)
    x[6] *= 1e-310
    x[7] *= 1e300
    pl = plan_for(n, c, 8)
    with np.errstate(all="ignore"):
        want = want_Y(x, c)
        got = pl.symbols(x)
        assert same_bits(got, want)
        assert not np.isfinite(want[2, 1]).any() and np.isnan(want[4, 2].real).all() and not want[0].any()
        x32 = x.astype(np.float32)
        x32[5] = np.float32(1e-45) * rng.integers(-3, 4, n).astype(np.float32)     # float32 denormals
        x32[6] = (rng.standard_normal(n) * 1e-40).astype(np.float32)
        assert np.any(x32[5] != 0) and np.any(x32[6] != 0)
        assert same_bits(pl.symbols(x32), want_Y(x32, c))
    xi = np.zeros((2, n), np.int16)
    xi[1, ::7] = [-32768, 32767] * 23
    assert same_bits(pl.symbols(xi), want_Y(xi, c))


# ---- 2. the slicer and the soft stage alone -------------------------------------------------
def want_bits(Y):
    return np.stack([oc.slice_bits(y) for y in Y])


def want_soft(Y):
    return np.stack([oc.soft(y) for y in Y])


def test_slice_and_soft_stage_sizes():
    """1 .. 131 products per stream: a word's 16 products and k_ofdm_soft's 256-thread block, short and exact."""
    import _amr
    rng = np.random.default_rng(20)
    for K, steps in ((1, [1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 131]), (3, [1, 5, 6, 11, 43, 44]),
                     (8, [1, 2, 3, 4, 16, 17]), (64, [1, 4, 5])):
        for nd in steps:
            for B in (1, 3, 65):
                Y = rng.standard_normal((B, nd + 1, K)) + 1j * rng.standard_normal((B, nd + 1, K))
                bits, soft = _amr.ofdm_slice(Y), _amr.ofdm_soft(Y)
                assert bits.shape == (B, 2 * K * nd) and np.array_equal(bits, want_bits(Y)), (K, nd, B)
                assert soft.dtype == np.int8 and np.array_equal(soft, want_soft(Y)), (K, nd, B)
                assert np.array_equal(soft > 0, bits.astype(bool))                       # the sign is the hard bit
    assert _amr.ofdm_slice(np.ones((3, 1, 8), np.complex128)).shape == (3, 0)            # S = 1: nothing
    assert _amr.ofdm_soft(np.ones((3, 1, 8), np.complex128)).shape == (3, 0)


def crafted_products():
    """|dr| == |di| exactly and one ulp to each side in the four diagonal directions; zeros, denormals,
    2^+-500, infinities and NaN in either component."""
    rng = np.random.default_rng(21)
    a = np.concatenate([10.0 ** rng.uniform(-3, 3, 40), [1.0, 0.75, 3.0, 2.0 ** -500, 2.0 ** 500]])
    d = []
    for other in (a, np.nextafter(a, 0.0), np.nextafter(a, np.inf)):
        for sr in (1.0, -1.0):
            for si in (1.0, -1.0):
                d.append(sr * a + 1j * si * other)
                d.append(sr * other + 1j * si * a)
    v = [0.0, -0.0, 5e-324, -5e-324, 2.0 ** -500, -2.0 ** -500, 2.0 ** 500, -2.0 ** 500, np.inf, -np.inf, np.nan, 1.0,
         -1.0]
    d.append(np.array([complex(x, y) for x in v for y in v]))
    return np.concatenate(d)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_ties_and_special_products(K):
    import _amr
    d = crafted_products()
    d = np.concatenate([d, np.ones(-d.size % K)])
    # symbol 0 is all ones, so the product of (1, d) is d itself wherever d is finite: the cases decide what they say
    Y = np.stack([np.ones(d.size), d]).reshape(2, -1, K)       # [2][q][K]: q pairs of symbols, each K wide
    Y = np.ascontiguousarray(Y.transpose(1, 0, 2))             # [q streams][S = 2][K]
    prod = np.concatenate([oc.products(y) for y in Y])
    fin = np.isfinite(d.real) & np.isfinite(d.imag)
    assert np.array_equal(prod[fin], d[fin]) and fin.sum() > 600
    m = oc.sectors(prod)[:24 * 45].reshape(3, 8, 45)         # [tie, an ulp less, an ulp more][direction][magnitude]
    assert set(m[0].ravel().tolist()) == {1, 3}              # an exact tie falls to the second line
    assert set(m[1, 0::2].ravel().tolist()) == {0, 2} and set(m[1, 1::2].ravel().tolist()) == {1, 3}
    assert set(m[2, 0::2].ravel().tolist()) == {1, 3} and set(m[2, 1::2].ravel().tolist()) == {0, 2}
    bits, soft = _amr.ofdm_slice(Y), _amr.ofdm_soft(Y)
    assert np.array_equal(bits, want_bits(Y)) and np.array_equal(soft, want_soft(Y))
    assert not np.any(soft == 0) and not np.any(soft == -128)
    # the same values along one stream's time axis: symbols 1, d, 1, d' ... give d, conj(d), d' ...
    Z = np.ones((1, 2 * (d.size // K), K), np.complex128)
    Z[0, 1::2] = d.reshape(-1, K)
    assert np.array_equal(_amr.ofdm_slice(Z), want_bits(Z)) and np.array_equal(_amr.ofdm_soft(Z), want_soft(Z))


# ---- 3. full demodulation -----------------------------------------------------------------
CASES = {"k8": (9600, 12000.0, 8, 96000, 4173), "k3": (19200, 24000.0, 3, 96000, 2111)}      # ..., n
B_MAX = 67
_cases = {}


def make_batch(name, dt):
    """[B_MAX][n] streams: payloads whose sync word sits 0 and 1 bits into a dibit, and noise alone."""
    baud, carrier, K, fs, n = CASES[name]
    rng = np.random.default_rng(n)
    L = K * int(fs / baud)
    room = (2 * K * (n // L - 1) - 80) // 8 - 4
    assert room >= 8
    rows = []
    for i in range(B_MAX):
        body = b"FB" + rng.integers(0, 256, room, dtype=np.uint8).tobytes()
        if i % 3 == 2:
            x = np.zeros(n, np.float32)
        else:
            shift = (i // 3) % 2
            bits = np.concatenate([np.zeros(shift, np.uint8), np.unpackbits(np.frombuffer(body, np.uint8)),
                                   np.zeros(8 - shift, np.uint8)])
            w = oc.modulate(np.packbits(bits).tobytes(), baud, carrier, K, fs)
            x = np.concatenate([w, np.zeros(max(0, n - w.size), np.float32)])[:n]
        rows.append(x + rng.normal(0, 0.04, n))
    x = np.stack(rows)
    if dt == "i16":
        return np.round(np.clip(x, -3.9, 3.9) * 8000).astype(np.int16)
    return x.astype(np.float32 if dt == "f32" else np.float64)


def case(name, dt):
    """(x, [(bytes, soft, sync)] from the restatement), computed once per module."""
    if (name, dt) not in _cases:
        x = make_batch(name, dt)
        _cases[name, dt] = (x, [oc.demod_soft(r, *CASES[name][:4]) for r in x])
    return _cases[name, dt]


def test_the_cases_hold_what_they_should():
    for name in CASES:
        x, want = case(name, "f32")
        syncs = np.array([w[2] for w in want])
        assert all(np.sum((syncs >= 0) & (syncs % 2 == r)) >= 15 for r in range(2)), (name, syncs)
        assert np.sum(syncs < 0) >= 15 and all(len(w[0]) > 0 for w in want), name
        assert all(oc.demod(r, *CASES[name][:4]) == (w[0], w[2]) for r, w in zip(x[:4], want))


@pytest.mark.parametrize("dt", ["f32", "f64", "i16"])
@pytest.mark.parametrize("name", list(CASES))
def test_demod_equals_the_restatement(name, dt):
    import _amr
    baud, carrier, K, fs, n = CASES[name]
    x, want = case(name, dt)
    for B in (1, 3, B_MAX):
        pl = _amr.OfdmPlan(n, baud, carrier, K, fs, max_streams=B)
        assert pl.out_cap == 2 * K * (n // (K * int(fs / baud)) - 1) // 8 + 1
        outs, sync = pl.demod_host(x[:B])
        assert outs == [w[0] for w in want[:B]], (name, dt, B)
        assert list(sync) == [w[2] for w in want[:B]], (name, dt, B)
    # more streams than the plan holds: the host layer cuts the batch
    pl = _amr.OfdmPlan(n, baud, carrier, K, fs, max_streams=16)
    assert pl.demod_host(x)[0] == [w[0] for w in want]


@pytest.mark.parametrize("name", list(CASES))
def test_demod_soft_equals_the_restatement(name):
    import _amr
    baud, carrier, K, fs, n = CASES[name]
    x, want = case(name, "f32")
    for B in (2, B_MAX):
        pl = _amr.OfdmPlan(n, baud, carrier, K, fs, max_streams=B)
        hard = pl.demod_host(x[:B])
        outs, sync, softs = pl.demod_soft_host(x[:B])
        assert outs == hard[0] and np.array_equal(sync, hard[1])
        for i, (data, soft, sy) in enumerate(want[:B]):
            assert outs[i] == data and sync[i] == sy, (name, B, i)
            assert softs[i].dtype == np.int8 and np.array_equal(softs[i], soft), (name, B, i)
            assert np.packbits(softs[i] > 0).tobytes() == outs[i], (name, B, i)


def test_modem_functions_plan_cache_and_timings():
    import _amr
    import modem
    baud, carrier, K, fs, n = CASES["k8"]
    x, want = case("k8", "f32")
    outs = modem.ofdm_demodulate_batch(x[:9], baud, carrier, K)
    assert outs == [w[0] for w in want[:9]]
    assert modem.ofdm_demodulate(x[1], baud, carrier, K) == want[1][0]
    x16 = x[1].astype(np.float16)                            # anything but float32 / float64 / int16 goes as float64
    assert modem.ofdm_demodulate(x16, baud, carrier, K) == oc.demod(x16, baud, carrier, K)[0]
    so, sv = modem.ofdm_demodulate_soft_batch(x[:9], baud, carrier, K)
    assert so == outs and all(np.array_equal(a, w[1]) for a, w in zip(sv, want))
    d1, s1 = modem.ofdm_demodulate_soft(x[4], baud, carrier, K)
    assert d1 == want[4][0] and np.array_equal(s1, want[4][1])
    pl = _amr.get_ofdm_plan(n, baud, carrier, K, fs, 9)
    assert pl is _amr.get_ofdm_plan(n, baud, carrier, K, fs, 3) and pl.max_streams == 16
    assert 0 < pl.scratch_bytes() <= _amr.lib().amr_ofdm_plan_bytes_estimate(n, 10, K, 16)
    pl.enable_timing()
    pl.demod_host(x[:9])
    t = pl.timings()
    assert set(t) == {"dft", "slice", "sync_pack", "launch"} and all(v >= 0 for v in t.values())
    assert t["launch"] >= max(t["dft"], t["slice"], t["sync_pack"])
    pl.enable_timing(False)
    # the aliases stay the reference's QPSK
    assert modem.ofdm_demodulate_simple(x[0], baud, carrier, K) == modem.qpsk_demodulate(x[0], baud, carrier)


def test_fewer_than_two_symbols_is_empty():
    import _amr
    import modem
    rng = np.random.default_rng(1)
    for n in (0, 79, 80, 159):                               # S = 0, 0, 1, 1 at L = 80
        x = rng.normal(0, 0.3, (3, n)).astype(np.float32)
        pl = _amr.OfdmPlan(n, 9600, 12000.0, 8, max_streams=3)
        assert pl.out_cap == 1
        outs, sync = pl.demod_host(x)
        assert outs == [b""] * 3 and list(sync) == [-1] * 3
        outs, sync, softs = pl.demod_soft_host(x)
        assert outs == [b""] * 3 and list(sync) == [-1] * 3 and all(s.size == 0 for s in softs)
        assert oc.demod(x[0], 9600, 12000.0, 8) == (b"", -1)
    assert modem.ofdm_demodulate(np.zeros(100, np.float32), 9600, 12000.0, 8) == b""
    assert modem.ofdm_demodulate_batch(np.zeros((0, 100), np.float32), 9600, 12000.0, 8) == []
    assert modem.ofdm_demodulate_soft_batch(np.zeros((0, 100), np.float32), 9600, 12000.0, 8) == ([], [])


def test_device_entries():
    """amr_ofdm_demod_device / _soft_device on the caller's buffers: wider rows, the soft rows pre-filled."""
    import _amr
    baud, carrier, K, fs, n = CASES["k8"]
    x, want = case("k8", "f32")
    B = 65
    L = _amr.lib()
    pl = _amr.OfdmPlan(n, baud, carrier, K, fs, max_streams=B)
    cap = pl.out_cap
    xw = np.zeros((B, n + 9), np.float32)
    xw[:, :n] = x[:B]
    with Dev() as d:
        d_x = d.put(xw)
        d_out, d_len, d_sync = d.put(np.zeros((B, cap + 3), np.uint8)), d.put(np.zeros(B, np.int64)), d.put(np.zeros(B, np.int64))
        d_soft = d.put(np.full((B, 8 * cap + 5), 77, np.int8))
        _amr.check(L.amr_ofdm_demod_device(pl.handle, d_x, _amr.DTYPE_F32, B, n + 9, d_out, cap + 3, d_len, d_sync))
        pl.synchronize()
        out, ln, sy = d.get(d_out, np.zeros((B, cap + 3), np.uint8)), d.get(d_len, np.zeros(B, np.int64)), d.get(d_sync, np.zeros(B, np.int64))
        assert [out[i, :ln[i]].tobytes() for i in range(B)] == [w[0] for w in want[:B]] and list(sy) == [w[2] for w in want[:B]]
        _amr.check(L.amr_ofdm_demod_soft_device(pl.handle, d_x, _amr.DTYPE_F32, B, n + 9, d_out, cap + 3, d_len, d_sync,
                                                d_soft, 8 * cap + 5))
        pl.synchronize()
        soft, ln2 = d.get(d_soft, np.zeros((B, 8 * cap + 5), np.int8)), d.get(d_len, np.zeros(B, np.int64))
        assert np.array_equal(ln, ln2)
        for i in range(B):
            assert np.array_equal(soft[i, :8 * ln[i]], want[i][1]), i
            assert np.all(soft[i, 8 * ln[i]:] == 77), i      # nothing past the stream's bytes is written
        # the argument contract, on a live plan
        assert L.amr_ofdm_demod_device(pl.handle, d_x, _amr.DTYPE_F32, B + 1, n + 9, d_out, cap + 3, d_len, d_sync) == _amr.AMR_E_CAPACITY
        assert L.amr_ofdm_demod_device(pl.handle, d_x, 7, B, n + 9, d_out, cap + 3, d_len, d_sync) == _amr.AMR_E_INVALID
        assert L.amr_ofdm_demod_device(pl.handle, d_x, _amr.DTYPE_F32, B, n - 1, d_out, cap + 3, d_len, d_sync) == _amr.AMR_E_INVALID
        assert L.amr_ofdm_demod_device(pl.handle, d_x, _amr.DTYPE_F32, B, n + 9, d_out, cap - 2, d_len, d_sync) == _amr.AMR_E_INVALID
        assert L.amr_ofdm_demod_soft_device(pl.handle, d_x, _amr.DTYPE_F32, B, n + 9, d_out, cap + 3, d_len, d_sync,
                                            d_soft, 8 * cap - 1) == _amr.AMR_E_INVALID
        assert L.amr_ofdm_demod_device(pl.handle, d_x, _amr.DTYPE_F32, 0, n + 9, d_out, cap + 3, d_len, d_sync) == _amr.AMR_OK


# ---- 4. transmit ----------------------------------------------------------------------------
TX_LENS = [0, 1, 2, 3, 5, 17, 64, 97]
_tx = {}


def tx_case(baud, K):
    """(payloads, the restatement's waveforms, [(n_out, want, got, pcm)]) of one configuration, computed once."""
    if (baud, K) not in _tx:
        import modem
        rng = np.random.default_rng(baud + K)
        datas = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in TX_LENS]
        L = K * (96000 // baud)
        refs = [oc.modulate(d, baud, 24000.0, K) for d in datas]
        assert [r.size for r in refs] == [oc.n_symbols(k, K) * L for k in TX_LENS]
        natural = max(r.size for r in refs)
        runs = []
        for n_out in (None, natural - 2 * L - 3, natural + 37):      # the natural length, shorter, longer
            want = np.zeros((len(datas), natural if n_out is None else n_out), np.float32)
            for i, r in enumerate(refs):
                k = min(r.size, want.shape[1])
                want[i, :k] = r[:k]
            got, pcm = modem.modulate_batch("ofdm", datas, baud, 24000.0, n_out=n_out, pcm=True, num_subcarriers=K)
            runs.append((n_out, want, got, pcm))
        _tx[baud, K] = (datas, refs, runs)
    return _tx[baud, K]


def within_one_ulp_per_sine(got, want, what=""):
    """|got - want| <= 2^-51 + one float32 ulp of want.  Each of a sample's K sines is within an ulp of the
    true value on either side, so the two differ by at most 2 * 2^-53 per sine (|sin| <= 1); K of them and the
    K sums' own roundings stay under K * 2^-51, which the factor 1 / K brings to 2^-51; the float32 cast of two
    doubles that close gives values at most that and one float32 ulp apart."""
    assert got.shape == want.shape and got.dtype == np.float32, what
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = 2.0 ** -51 + np.spacing(np.abs(want)).astype(np.float64)
    assert np.all(diff <= bound), (what, float(diff.max()))


@pytest.mark.parametrize("K", [1, 3, 8, 64])
@pytest.mark.parametrize("baud", [19200, 9600, 1200])        # sps 5, 10, 80
def test_modulate_batch_equals_the_restatement(baud, K):
    """The rule set for the modulator: test_gpu_tx.assert_close, at most one float32 ulp from the restatement
    and at most 1 + 1e-6 x size samples that differ at all.  Figures of each run are printed before the assertion.

    Where a sample's K sines cancel (|value| <= 3.5e-14 of a full scale of 1), the last ulp of one sine is the
    whole sample: with a sine that is only within an ulp, 5 of these 12 cases missed the rule on an MI355X
    (K = 3 at every rate, K = 8 and 64 at 1200 Bd: 48 to 109 samples each, |got - want| <= 5.6e-17 but 6e8
    float32 ulps).  The kernel's sines are correctly rounded for that reason (ofdm_sin_cr), as
    numpy's are for all but about one argument in 700; with them no sample of the 12 cases differs at all."""
    import modem
    datas, refs, runs = tx_case(baud, K)
    for n_out, want, got, pcm in runs:
        u = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        far = u > 1
        print(f"ofdm tx baud {baud} K {K} n_out {n_out}: {got.size} samples, {np.count_nonzero(u)} differ, "
              f"{np.count_nonzero(far)} by more than one float32 ulp; max |got - want| "
              f"{np.abs(got.astype(np.float64) - want).max():.3e}, largest |want| among those "
              f"{np.abs(want[far]).max(initial=0.0):.3e}")
    for n_out, want, got, pcm in runs:
        assert_close(got, want, pcm, (want * np.float32(32767)).astype(np.int16), (baud, K, n_out))
    one = modem.ofdm_modulate(datas[5], baud, 24000.0, K)
    assert_close(one, refs[5], what=(baud, K, "single"))


@pytest.mark.parametrize("K", [1, 3, 8, 64])
@pytest.mark.parametrize("baud", [19200, 9600, 1200])
def test_modulate_batch_within_one_ulp_per_sine(baud, K):
    """The same waveforms under the bound the definition itself gives (within_one_ulp_per_sine), the padding
    exact zeros, the int16 samples those of the float32 ones; and the aliases stay the reference's QPSK."""
    import modem
    datas, refs, runs = tx_case(baud, K)
    for n_out, want, got, pcm in runs:
        within_one_ulp_per_sine(got, want, (baud, K, n_out))
        for i, r in enumerate(refs):
            assert not got[i, r.size:].any(), (baud, K, n_out, i)
        assert np.array_equal(pcm, (got * np.float32(32767)).astype(np.int16)), (baud, K, n_out)
    if baud != 19200:                                        # (19200 Bd is the QPSK modulator's empty-ramp ValueError)
        assert np.array_equal(modem.ofdm_modulate_simple(datas[3], baud, 24000.0, K),
                              modem.qpsk_modulate(datas[3], baud, 24000.0))


# ---- 5. loopback and the coded chain --------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.0, 0.05])
@pytest.mark.parametrize("K", [1, 3, 4, 8])
@pytest.mark.parametrize("baud,carrier", oc.CONFIGS)
def test_loopback_frames_parse(baud, carrier, K, sigma):
    """GPU modulator -> noise -> GPU demodulator -> frame scan: every frame's payload comes back, CRC valid."""
    import modem
    from test_gpu_loopback import _frames, _payloads, _want_payload
    rng = np.random.default_rng(baud + K)
    frames = _frames(4, 48, seed=baud + K)
    x = modem.modulate_batch("ofdm", frames, baud, carrier, num_subcarriers=K)
    if sigma:
        x = x + rng.normal(0, sigma, x.shape).astype(np.float32)
    raws = modem.ofdm_demodulate_batch(x, baud, carrier, K)
    got = _payloads(raws)
    for i, fr in enumerate(frames):
        assert raws[i][:len(fr)] == fr and got[i] == [_want_payload(fr)], (baud, K, sigma, i)


@pytest.mark.parametrize("K", [16, 64])
def test_loopback_many_subcarriers_clean(K):
    import modem
    from test_gpu_loopback import _frames
    frames = _frames(3, 48, seed=K)
    x = modem.modulate_batch("ofdm", frames, 9600, 12000.0, num_subcarriers=K)
    raws = modem.ofdm_demodulate_batch(x, 9600, 12000.0, K)
    assert all(r[:len(f)] == f for r, f in zip(raws, frames))
    # a capture that starts Ncp samples late decodes to the same bytes
    Ncp = oc.geometry(9600, 12000.0, K)[2]
    late = np.concatenate([np.zeros((3, Ncp), np.float32), x], axis=1)
    assert modem.ofdm_demodulate_batch(late, 9600, 12000.0, K) == raws


def test_end_to_end_coded_chain():
    """encode_batch -> ofdm modulate -> noise -> ofdm soft demodulation -> decode_soft_batch returns the
    messages.  9600 Bd on a 12 kHz carrier, 8 subcarriers, 16 messages of 120 bytes, N(0, 0.14^2) on the
    samples (seed 8): the level was picked by running this chain's restatement on the CPU
    (ofdm_cases.modulate -> demod_soft -> soft_cases.soft_decode_batch) at 0.10 .. 0.35 with seeds 7, 8, 9.
    The uncoded 16-bit sync word sets the limit here: with 24-byte messages it is lost in some of the 16
    streams (from 0.16 on) before every 50-byte codeword is damaged, so the messages are 120 bytes; at 0.14
    and seed 8 every one of the 16 received 242-byte codewords has byte errors, the sync word is found in all
    16 streams and the soft decoder returns all 16 messages (at 0.15 two streams lose the sync).  The
    restatement runs here again, so the GPU's soft values are checked at this level too."""
    import fec
    import modem
    rng = np.random.default_rng(8)
    msgs = vc.messages(rng, [120] * 16)
    cws = fec.ConvolutionalEncoder().encode_batch(msgs)
    L = len(cws[0])
    assert L == 242 and cws == [vc.encode(m) for m in msgs]
    tx = modem.modulate_batch("ofdm", [b"FB" + c for c in cws], baud=9600, f0=12000.0, num_subcarriers=8)
    ref = np.stack([oc.modulate(b"FB" + c, 9600, 12000.0, 8) for c in cws])
    within_one_ulp_per_sine(tx, ref, "coded chain")          # the level was picked on the restatement's samples
    x = (tx.astype(np.float64) + rng.normal(0, 0.14, tx.shape)).astype(np.float32)
    outs, softs = modem.ofdm_demodulate_soft_batch(x, 9600, 12000.0, 8)
    want = [oc.demod_soft(r, 9600, 12000.0, 8) for r in x]
    assert outs == [w[0] for w in want] and all(np.array_equal(s, w[1]) for s, w in zip(softs, want))
    assert all(o[:2] == b"FB" and len(o) >= 2 + L for o in outs)          # sync found in all
    assert all(o[2:2 + L] != c for o, c in zip(outs, cws))                # and every hard codeword is damaged
    rows = [s[16:16 + 8 * L] for s in softs]
    assert [m for m, _ in sc.soft_decode_batch(rows)] == msgs
    assert fec.ViterbiDecoder().decode_soft_batch(rows) == msgs
