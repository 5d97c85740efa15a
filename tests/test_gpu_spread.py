"""spread on the GPU: k_dsss_despread, k_dsss_acquire, k_dsss_acq_max,
k_dsss_slice, k_dsss_soft and the transmit kernels (dsss_kernels.hip,
dsss_acq_kernels.hip) with the plan / host layer around them, against the numpy
restatement in tests/spread_cases.py: bit-equal throughout, the transmit
samples included."""
import numpy as np
import pytest

import soft_cases as sc
import spread_cases as sp
import viterbi_cases as vc
from test_gpu_ofdm import same_bits
from test_gpu_viterbi import Dev

pytestmark = pytest.mark.gpu

# (C, spc): L = 3, 15, 91, 80, 160, 640, 1280 -- below a wave, not dividing 64, above a block; 640 and 1280 are
# two and three tiles of offsets in k_dsss_acquire, 1280 takes its chips in two steps
GEOS = [(3, 1), (3, 5), (13, 7), (16, 5), (16, 10), (64, 10), (16, 80)]
BIG = (64, 80)            # L = 5120: ten tiles, chips in steps of 7; M <= 3 and 2 streams only (the restatement's time)
LONG_CHIP = (3, 200)      # L = 600, spc above the staged-product limit: the chip sums straight from x
MOD4 = [(3, 3), (2, 5)]   # L = 9, 10: with the others L mod 4 = 0, 1, 2, 3
SYMBOLS = [0, 1, 2, 63, 64, 65]
STREAMS = [1, 2, 65]


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")
    assert "amr_dsss_plan_create" in _amr.EXPORTS            # the restatement is only worth testing beside the product


def code_of(C):
    import _amr
    return {2: [1, 0], 3: [1, 0, 0], 13: sp.CODE13, 16: _amr.DSSS_CODE, 64: sp.code64()}[C]


def cfg(C, spc):
    """(baud, carrier, code, samp_rate) with exactly spc samples per chip and the carrier at fs / 4:
    cyc = floor(L / 4 + 0.5), valid from L = 3 on."""
    fs = 1000 * spc
    return 1000, fs / 4.0, code_of(C), fs


def plan_for(n, c, B):
    import _amr
    baud, carrier, code, fs = c
    return _amr.DsssPlan(n, baud, carrier, code, fs, max_streams=B)


def want_Y(x, c, offs=None):
    offs = np.zeros(len(x), np.int64) if offs is None else offs
    return np.stack([sp.symbols(r, o, *c) for r, o in zip(x, offs)])


def want_acq(x, c):
    got = [sp.acquire(r, *c) for r in x]
    return np.array([g[0] for g in got], np.int64), np.stack([g[1] for g in got])


def test_the_geometries_cover_what_they_should():
    Ls = [sp.geometry(*cfg(C, spc))[1] for C, spc in GEOS + MOD4 + [BIG, LONG_CHIP]]
    assert Ls == [3, 15, 91, 80, 160, 640, 1280, 9, 10, 5120, 600] and {L % 4 for L in Ls} == {0, 1, 2, 3}
    for C, spc in GEOS + MOD4 + [BIG, LONG_CHIP]:
        spc_, L, cyc, code = sp.geometry(*cfg(C, spc))
        assert spc_ == spc and 1 <= cyc and 2 * cyc < L


# ---- 1. the despreader alone ----------------------------------------------------------------
@pytest.mark.parametrize("C,spc", GEOS + MOD4 + [LONG_CHIP])
def test_despread_geometries_and_offsets(C, spc):
    """Offsets 0, 1, L - 1 and mixed per stream: the last row of a stream read from o > tail is cut at n."""
    c = cfg(C, spc)
    L = C * spc
    rng = np.random.default_rng(100 * C + spc)
    x = rng.standard_normal((4, 5 * L + 1)).astype(np.float32)
    pl = plan_for(x.shape[1], c, 4)
    got = pl.symbols_at(x)
    assert got.shape == (4, 5) and same_bits(got, want_Y(x, c))
    assert np.abs(got).max() > 0.5                           # not the zeros of a kernel that did not run
    for offs in ([0] * 4, [1] * 4, [L - 1] * 4, [L - 1, 0, 1, L // 2]):
        offs = np.array(offs, np.int64)
        assert same_bits(pl.symbols_at(x, offs), want_Y(x, c, offs)), offs
    for bad in (-1, L):
        with pytest.raises(Exception):
            pl.symbols_at(x, np.array([0, bad, 0, 0], np.int64))


def test_despread_the_longest_bit():
    C, spc = BIG
    c = cfg(C, spc)
    L = C * spc
    rng = np.random.default_rng(5120)
    x = rng.standard_normal((2, 3 * L + 7)).astype(np.float32)
    pl = plan_for(x.shape[1], c, 2)
    offs = np.array([L - 1, 8], np.int64)
    assert same_bits(pl.symbols_at(x), want_Y(x, c)) and same_bits(pl.symbols_at(x, offs), want_Y(x, c, offs))


@pytest.mark.parametrize("S", SYMBOLS)
@pytest.mark.parametrize("C,spc", [(16, 5), (3, 5)])
def test_despread_symbol_and_stream_counts(C, spc, S):
    """Flat bit indices b*S + s cross wave edges inside and between streams; a partial tail of 0, 1 and L - 1
    samples is ignored at offset 0 and read, as far as it goes, at an offset."""
    c = cfg(C, spc)
    L = C * spc
    rng = np.random.default_rng(1000 * C + S)
    for B, r in zip(STREAMS, (0, 1, L - 1)):
        n = S * L + r
        x = rng.standard_normal((B, n)).astype(np.float32)
        pl = plan_for(n, c, B)
        assert pl.S == S
        got = pl.symbols_at(x)
        assert got.shape == (B, S), (B, r)
        if S:
            assert same_bits(got, want_Y(x, c)), (B, r)
            offs = rng.integers(0, L, B)
            assert same_bits(pl.symbols_at(x, offs), want_Y(x, c, offs)), (B, r)
    # a plan larger than the batch, and a second call on it
    pl = plan_for(S * L + 2, c, 70)
    x = rng.standard_normal((3, S * L + 2))
    for _ in range(2):
        got = pl.symbols_at(x)
        assert got.shape == (3, S) and (S == 0 or same_bits(got, want_Y(x, c)))


@pytest.mark.parametrize("dt", ["f32", "f64", "i16"])
def test_despread_dtypes_and_row_stride(dt):
    c = cfg(16, 10)
    n = 7 * 160 + 5
    rng = np.random.default_rng(3)
    wide = rng.standard_normal((5, n + 13))
    wide = np.round(wide * 9000).astype(np.int16) if dt == "i16" else wide.astype({"f32": np.float32, "f64": np.float64}[dt])
    x = wide[:, :n]                                          # rows of a wider array: x_stride = n + 13
    assert x.strides[0] == (n + 13) * x.itemsize
    pl = plan_for(n, c, 8)
    offs = np.array([0, 159, 6, 5, 4], np.int64)             # 159 and 6 pass n in the last row: not the padding's samples
    assert same_bits(pl.symbols_at(x), want_Y(x, c)) and same_bits(pl.symbols_at(x, offs), want_Y(x, c, offs))
    assert same_bits(pl.symbols_at(np.ascontiguousarray(x), offs), want_Y(x, c, offs))


def test_despread_special_samples():
    """+-inf, NaN, denormals and all zeros: float64 arithmetic has one answer for each (a NaN's sign aside)."""
    c = cfg(16, 5)
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
    offs = np.array([3, 0, 17, 79, 41, 2, 1, 0], np.int64)
    with np.errstate(all="ignore"):
        want = want_Y(x, c)
        assert same_bits(pl.symbols_at(x), want) and same_bits(pl.symbols_at(x, offs), want_Y(x, c, offs))
        assert not np.isfinite(want[2, 1].real) and np.isnan(want[4, 2].real) and not want[0].any()
        x32 = x.astype(np.float32)
        x32[5] = np.float32(1e-45) * rng.integers(-3, 4, n).astype(np.float32)     # float32 denormals
        assert np.any(x32[5] != 0)
        assert same_bits(pl.symbols_at(x32, offs), want_Y(x32, c, offs))
    xi = np.zeros((2, n), np.int16)
    xi[1, ::7] = [-32768, 32767] * 23
    assert same_bits(pl.symbols_at(xi), want_Y(xi, c))


# ---- 2. acquisition alone ---------------------------------------------------------------------
def check_acquire(x, c, B=None):
    pl = plan_for(x.shape[1], c, B or len(x))
    off, P = pl.acquire(x)
    woff, wP = want_acq(x, c)
    assert P.shape == wP.shape and same_bits(P, wP)
    assert np.array_equal(off, woff), (off, woff)
    return off, P


@pytest.mark.parametrize("C,spc", GEOS + MOD4 + [LONG_CHIP])
def test_acquire_geometries(C, spc):
    c = cfg(C, spc)
    L = C * spc
    rng = np.random.default_rng(7 * C + spc)
    x = rng.standard_normal((3, 4 * L + L // 2)).astype(np.float32)      # M = 3
    assert sp.acq_bits(x.shape[1], L) == 3
    off, P = check_acquire(x, c)
    assert P.min() > 0.0                                     # every offset was written
    # a frame at a delay is found to the sample (C >= 13: three chips correlate with anything)
    if C >= 13:
        t = int(rng.integers(1, L))
        y = sp.delayed(b"FB" + bytes(3), t, *c[:3], samp_rate=c[3])[None, :]
        assert check_acquire(y, c)[0][0] == t


def test_acquire_the_longest_bit():
    """L = 5120: the offsets in ten tiles, the 64 chips in steps of 7 with y carried across them."""
    C, spc = BIG
    c = cfg(C, spc)
    L = C * spc
    rng = np.random.default_rng(5121)
    x = rng.standard_normal((2, 4 * L - 1)).astype(np.float32)           # M = 3, the last sample read is n - 1
    x[1, 777:777 + 2 * L] += 3 * sp.modulate(b"", *c[:3], samp_rate=c[3])[:2 * L]
    off, P = check_acquire(x, c)
    assert abs(int(off[1]) - 777) <= 1                       # two bits under noise: within a sample


@pytest.mark.parametrize("M", [0, 1, 2, 63, 64, 65, 129])
@pytest.mark.parametrize("C,spc", [(16, 5), (3, 5)])
def test_acquire_bit_and_stream_counts(C, spc, M):
    """Segments of 64 bits: none, a partial one, a whole one, one and a bit, two and a bit; (n - L + 1) % L = 0, 1
    and L - 1, the last of which reads the capture's last sample."""
    c = cfg(C, spc)
    L = C * spc
    rng = np.random.default_rng(100 * M + C)
    for B, r in zip(STREAMS, (0, 1, L - 1)):
        n = (M + 1) * L - 1 + r if M else (0, 1, 2 * L - 2)[STREAMS.index(B)]
        assert sp.acq_bits(n, L) == M and (M == 0 or (n - L + 1) % L == r)
        x = rng.standard_normal((B, n)).astype(np.float32)
        off, P = check_acquire(x, c)
        if M == 0:
            assert not P.any() and not off.any()
    x = rng.standard_normal((3, (M + 1) * L + 2))            # a plan larger than the batch, twice, float64
    pl = plan_for(x.shape[1], c, 70)
    for _ in range(2):
        off, P = pl.acquire(x)
        woff, wP = want_acq(x, c)
        assert same_bits(P, wP) and np.array_equal(off, woff)


@pytest.mark.parametrize("dt", ["f32", "f64", "i16"])
def test_acquire_dtypes_row_stride_and_device_entry(dt):
    import _amr
    c = cfg(16, 10)
    L = 160
    n = 6 * L + 11
    rng = np.random.default_rng(31)
    wide = rng.standard_normal((5, n + 13))
    wide = np.round(wide * 9000).astype(np.int16) if dt == "i16" else wide.astype({"f32": np.float32, "f64": np.float64}[dt])
    x = wide[:, :n]
    off, P = check_acquire(x, c, 8)
    pl = plan_for(n, c, 8)
    lib = _amr.lib()
    with Dev() as d:
        d_x, d_off, d_P = d.put(wide), d.put(np.zeros(5, np.int64)), d.put(np.zeros((5, L)))
        _amr.check(lib.amr_dsss_acquire_device(pl.handle, d_x, _amr.DTYPES[x.dtype], 5, n + 13, d_off, d_P))
        pl.synchronize()
        assert np.array_equal(d.get(d_off, np.zeros(5, np.int64)), off) and same_bits(d.get(d_P, np.zeros((5, L))), P)
        _amr.check(lib.amr_dsss_acquire_device(pl.handle, d_x, _amr.DTYPES[x.dtype], 2, n + 13, d_off, None))   # P optional
        pl.synchronize()
        assert lib.amr_dsss_acquire_device(pl.handle, d_x, _amr.DTYPES[x.dtype], 9, n + 13, d_off, None) == _amr.AMR_E_CAPACITY
        assert lib.amr_dsss_acquire_device(pl.handle, d_x, 7, 5, n + 13, d_off, None) == _amr.AMR_E_INVALID
        assert lib.amr_dsss_acquire_device(pl.handle, d_x, _amr.DTYPES[x.dtype], 5, n - 1, d_off, None) == _amr.AMR_E_INVALID


def test_acquire_zeros_nan_and_ties():
    c = cfg(16, 10)
    L = 160
    rng = np.random.default_rng(32)
    n = 7 * L + 140
    M = sp.acq_bits(n, L)
    assert M == 6 and n - M * L > 101
    x = rng.standard_normal((6, n)).astype(np.float32)
    x[0] = 0.0                                               # all zeros: o = 0
    x[1, 0] = np.nan                                         # P[0] is NaN: 0 is kept
    x[2, M * L + 100] = np.nan                               # only the windows of d >= 101 hold it: NaN never wins
    x[3, 3 * L + 9] = np.inf
    # an exact tie: one sample alone, past the last whole bit, is in one window of each d >= 41 and in none of
    # the others; each of those P[d] is the same |x W|^2, bit for bit: the first index wins, across lanes too
    x[4] = 0.0
    x[4, M * L + 40] = 0.75
    x[5] = 0.0
    x[5, M * L + 140] = -1.5
    with np.errstate(all="ignore"):
        off, P = check_acquire(x, c)
    assert off[0] == 0 and not P[0].any()
    assert off[1] == 0 and np.isnan(P[1, 0])
    assert np.flatnonzero(np.isnan(P[2])).tolist() == list(range(101, L)) and off[2] < 101
    assert np.unique(P[4, 41:]).size == 1 and P[4, 41] > 0 and not P[4, :41].any() and off[4] == 41
    assert np.unique(P[5, 141:]).size == 1 and not P[5, :141].any() and off[5] == 141


# ---- 3. the slicer and the soft stage alone ---------------------------------------------------
def want_bits(Y):
    return np.stack([sp.slice_bits(y) for y in Y])


def want_soft(Y):
    return np.stack([sp.soft(y) for y in Y])


def test_slice_and_soft_stage_sizes():
    """1 .. 300 products per stream: a word's 32 bits, a wave's two words, k_dsss_soft's 256-thread block."""
    import _amr
    rng = np.random.default_rng(20)
    for nd in (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300):
        for B in (1, 3, 65):
            Y = rng.standard_normal((B, nd + 1)) + 1j * rng.standard_normal((B, nd + 1))
            bits, soft = _amr.dsss_slice(Y), _amr.dsss_soft(Y)
            assert bits.shape == (B, nd) and np.array_equal(bits, want_bits(Y)), (nd, B)
            assert soft.dtype == np.int8 and np.array_equal(soft, want_soft(Y)), (nd, B)
            assert np.array_equal(soft > 0, bits.astype(bool))                       # the sign is the hard bit
    assert _amr.dsss_slice(np.ones((3, 1), np.complex128)).shape == (3, 0)           # S = 1: nothing
    assert _amr.dsss_soft(np.ones((3, 1), np.complex128)).shape == (3, 0)


def test_special_products():
    """Exact zeros of either sign, dr an ulp to each side of 0, NaN, inf and 2^+-500 in either component."""
    import _amr
    tiny = 5e-324
    v = [0.0, -0.0, tiny, -tiny, 2.0 ** -500, -2.0 ** -500, 2.0 ** 500, -2.0 ** 500, np.inf, -np.inf, np.nan, 1.0, -1.0,
         np.nextafter(1.0, 2.0), -np.nextafter(1.0, 0.0)]
    d = np.array([complex(a, b) for a in v for b in v])
    # symbol 0 is 1, so the product of (1, d) is d itself wherever d is finite: the cases decide what they say
    Y = np.ascontiguousarray(np.stack([np.ones(d.size), d], axis=1))                 # [streams][S = 2]
    with np.errstate(all="ignore"):
        prod = np.concatenate([sc.diff_products(y) for y in Y])
        fin = np.isfinite(d.real) & np.isfinite(d.imag)
        assert np.array_equal(prod[fin], d[fin]) and fin.sum() > 100
        bits, soft = _amr.dsss_slice(Y), _amr.dsss_soft(Y)
        assert np.array_equal(bits, want_bits(Y)) and np.array_equal(soft, want_soft(Y))
        assert not np.any(soft == 0) and not np.any(soft == -128)
        assert np.array_equal(bits[fin, 0] == 1, d.real[fin] < 0)
        # the same values along one stream's time axis: symbols 1, d, 1, d' ... give d, conj(d), d' ...
        Z = np.ones((1, 2 * d.size), np.complex128)
        Z[0, 1::2] = d
        assert np.array_equal(_amr.dsss_slice(Z), want_bits(Z)) and np.array_equal(_amr.dsss_soft(Z), want_soft(Z))


# ---- 4. full demodulation -------------------------------------------------------------------
CASES = {"c16": (9600, 12000.0, None, 96000), "c13": (19200, 24000.0, sp.CODE13, 96000)}
B_MAX = 67
SHORT = 5                 # streams of the float64 and int16 batches (the restatement's time)
_cases = {}


def make_batch(name, dt):
    """[B][n] streams at random delays under N(0, 0.3^2): frames whose sync word sits 0 .. 7 bits into a byte,
    and noise alone (no sync word)."""
    baud, carrier, code, fs = CASES[name]
    rng = np.random.default_rng(len(name) + int(baud))
    L = sp.geometry(baud, carrier, code, fs)[1]
    room = 10
    n = (81 + 8 * (room + 3)) * L + 2 * L + 17
    rows = []
    for i in range(B_MAX if dt == "f32" else SHORT):
        x = np.zeros(n, np.float32)
        if i % 3 != 2:
            shift = (i // 3) % 8
            body = b"FB" + rng.integers(0, 256, room, dtype=np.uint8).tobytes()
            bits = np.concatenate([np.zeros(shift, np.uint8), np.unpackbits(np.frombuffer(body, np.uint8)),
                                   np.zeros(8 - shift, np.uint8)])
            w = sp.modulate(np.packbits(bits).tobytes(), baud, carrier, code, fs)
            t = int(rng.integers(0, L))
            x[t:t + w.size] = w
        rows.append(x + rng.normal(0, 0.3, n))
    x = np.stack(rows)
    if dt == "i16":
        return np.round(np.clip(x, -3.9, 3.9) * 8000).astype(np.int16)
    return x.astype(np.float32 if dt == "f32" else np.float64)


def case(name, dt):
    """(x, acquired [(bytes, soft, sync, o)], unacquired the same) from the restatement, computed once per module."""
    if (name, dt) not in _cases:
        x = make_batch(name, dt)
        c = CASES[name]
        _cases[name, dt] = (x, [sp.demod_soft(r, *c) for r in x], [sp.demod_soft(r, *c, acquire_=False) for r in x])
    return _cases[name, dt]


def test_the_cases_hold_what_they_should():
    for name in CASES:
        x, acq, plain = case(name, "f32")
        syncs = np.array([w[2] for w in acq])
        assert np.sum(syncs >= 0) >= 40 and np.sum(syncs < 0) >= 15 and all(len(w[0]) > 0 for w in acq), (name, syncs)
        assert len({int(s) % 8 for s in syncs if s >= 0}) == 8                   # every alignment of the sync word
        assert len({w[3] for w in acq}) > 20                                     # the delays differ
        assert sum(a[0] != p[0] for a, p in zip(acq, plain)) > 20                # and acquisition matters
        assert all(sp.demod(r, *CASES[name])[:2] == (w[0], w[2]) for r, w in zip(x[:3], acq))


@pytest.mark.parametrize("acquire", [True, False])
@pytest.mark.parametrize("dt", ["f32", "f64", "i16"])
@pytest.mark.parametrize("name", list(CASES))
def test_demod_equals_the_restatement(name, dt, acquire):
    import _amr
    baud, carrier, code, fs = CASES[name]
    x, acq, plain = case(name, dt)
    want = acq if acquire else plain
    n = x.shape[1]
    for B in sorted({1, 3, len(x)}):
        pl = _amr.DsssPlan(n, baud, carrier, code, fs, max_streams=B)
        assert pl.out_cap == (n // pl.L - 1) // 8 + 1
        outs, sync, softs, offs = pl.demod_host(x[:B], soft=True, acquire=acquire)
        assert outs == [w[0] for w in want[:B]], (name, dt, B)
        assert list(sync) == [w[2] for w in want[:B]] and list(offs) == [w[3] for w in want[:B]], (name, dt, B)
        for i, w in enumerate(want[:B]):
            assert softs[i].dtype == np.int8 and np.array_equal(softs[i], w[1]), (name, dt, B, i)
            assert np.packbits(softs[i] > 0).tobytes() == outs[i]
        hard = pl.demod_host(x[:B], acquire=acquire)
        assert hard[0] == outs and np.array_equal(hard[1], sync) and hard[2] is None and np.array_equal(hard[3], offs)
    # more streams than the plan holds: the host layer cuts the batch
    pl = _amr.DsssPlan(n, baud, carrier, code, fs, max_streams=4)
    assert pl.demod_host(x, acquire=acquire)[0] == [w[0] for w in want]


def test_modem_functions_plan_cache_and_timings():
    import _amr
    import modem
    baud, carrier, code, fs = CASES["c16"]
    x, acq, plain = case("c16", "f32")
    n = x.shape[1]
    assert modem.spread_demodulate_batch(x[:9], baud, carrier) == [w[0] for w in acq[:9]]
    assert modem.spread_demodulate_batch(x[:9], baud, carrier, acquire=False) == [w[0] for w in plain[:9]]
    assert modem.spread_demodulate(x[1], baud, carrier) == acq[1][0]
    assert list(modem.spread_acquire_batch(x[:9], baud, carrier)) == [w[3] for w in acq[:9]]
    assert modem.spread_acquire(x[4], baud, carrier) == acq[4][3]
    x16 = x[1].astype(np.float16)                            # anything but float32 / float64 / int16 goes as float64
    assert modem.spread_demodulate(x16, baud, carrier) == sp.demod(x16, baud, carrier)[0]
    so, sv = modem.spread_demodulate_soft_batch(x[:9], baud, carrier)
    assert so == [w[0] for w in acq[:9]] and all(np.array_equal(a, w[1]) for a, w in zip(sv, acq))
    d1, s1 = modem.spread_demodulate_soft(x[4], baud, carrier, acquire=False)
    assert d1 == plain[4][0] and np.array_equal(s1, plain[4][1])
    xc, acq13, _ = case("c13", "f32")
    assert modem.spread_demodulate(xc[0], 19200, 24000.0, code=sp.CODE13) == acq13[0][0]
    # the cache is keyed by the code too, and counts the acquisition buffers once a plan acquires
    pl = _amr.get_dsss_plan(n, baud, carrier, None, fs, 9)
    assert pl is _amr.get_dsss_plan(n, baud, carrier, _amr.DSSS_CODE, fs, 3) and pl.max_streams == 16
    assert pl is not _amr.get_dsss_plan(n, baud, carrier, [0] + _amr.DSSS_CODE[1:], fs, 3)
    lib = _amr.lib()
    total = lib.amr_dsss_plan_bytes_estimate(n, 10, 16, 16) + lib.amr_dsss_acquire_bytes_estimate(n, 10, 16, 16)
    assert lib.amr_dsss_acquire_bytes_estimate(n, 10, 16, 16) < pl.scratch_bytes() <= total
    fresh = _amr.DsssPlan(n, baud, carrier, None, fs, max_streams=4)
    before = fresh.scratch_bytes()
    fresh.demod_host(x[:4], acquire=False)
    staged = fresh.scratch_bytes()
    fresh.acquire(x[:4])
    assert before < staged and fresh.scratch_bytes() == staged + lib.amr_dsss_acquire_bytes_estimate(n, 10, 16, 4)
    pl.enable_timing()
    pl.demod_host(x[:9], acquire=False)
    t = pl.timings()
    assert set(t) == {"despread", "slice", "sync_pack", "launch"} and all(v >= 0 for v in t.values())
    pl.demod_host(x[:9], soft=True)
    t = pl.timings()
    assert set(t) == set(_amr.TD_SLOTS) and t["launch"] >= max(t["acquire"], t["despread"], t["slice"], t["sync_pack"])
    pl.enable_timing(False)
    # the alias stays the reference's BPSK
    assert np.array_equal(modem.dsss_modulate(b"FBPC", 9600, 12000.0), modem.bpsk_modulate(b"FBPC", 9600, 12000.0))


def test_fewer_than_two_bits_is_empty():
    import _amr
    import modem
    rng = np.random.default_rng(1)
    for n in (0, 159, 160, 319):                             # S = 0, 0, 1, 1 at L = 160
        x = rng.normal(0, 0.3, (3, n)).astype(np.float32)
        pl = _amr.DsssPlan(n, 9600, 12000.0, max_streams=3)
        assert pl.out_cap == 1
        for acquire in (False, True):
            outs, sync, softs, offs = pl.demod_host(x, soft=True, acquire=acquire)
            assert outs == [b""] * 3 and list(sync) == [-1] * 3 and all(s.size == 0 for s in softs)
            assert list(offs) == [sp.acquire(r, 9600, 12000.0)[0] if acquire else 0 for r in x]
        assert sp.demod(x[0], 9600, 12000.0)[:2] == (b"", -1)
    assert modem.spread_demodulate(np.zeros(100, np.float32), 9600, 12000.0) == b""


def test_device_entries():
    """amr_dsss_demod_device on the caller's buffers: wider rows, the soft rows pre-filled, soft and offset
    optional, acquired and not: the same bytes, values and offsets as the host entry."""
    import _amr
    baud, carrier, code, fs = CASES["c16"]
    x, acq, plain = case("c16", "f32")
    n = x.shape[1]
    B = 65
    L = _amr.lib()
    pl = _amr.DsssPlan(n, baud, carrier, code, fs, max_streams=B)
    cap = pl.out_cap
    xw = np.zeros((B, n + 9), np.float32)
    xw[:, :n] = x[:B]
    F32 = _amr.DTYPE_F32
    with Dev() as d:
        d_x = d.put(xw)
        d_out, d_len, d_sync = d.put(np.zeros((B, cap + 3), np.uint8)), d.put(np.zeros(B, np.int64)), d.put(np.zeros(B, np.int64))
        d_off = d.put(np.full(B, -5, np.int64))
        for acquire, want in ((1, acq), (0, plain)):
            d_soft = d.put(np.full((B, 8 * cap + 5), 77, np.int8))
            _amr.check(L.amr_dsss_demod_device(pl.handle, d_x, F32, B, n + 9, d_out, cap + 3, d_len, d_sync, d_soft,
                                               8 * cap + 5, d_off, acquire))
            pl.synchronize()
            out, ln, sy = d.get(d_out, np.zeros((B, cap + 3), np.uint8)), d.get(d_len, np.zeros(B, np.int64)), d.get(d_sync, np.zeros(B, np.int64))
            assert [out[i, :ln[i]].tobytes() for i in range(B)] == [w[0] for w in want[:B]]
            assert list(sy) == [w[2] for w in want[:B]]
            assert list(d.get(d_off, np.zeros(B, np.int64))) == [w[3] for w in want[:B]]
            soft = d.get(d_soft, np.zeros((B, 8 * cap + 5), np.int8))
            for i in range(B):
                assert np.array_equal(soft[i, :8 * ln[i]], want[i][1]), i
                assert np.all(soft[i, 8 * ln[i]:] == 77), i      # nothing past the stream's bytes is written
            # soft and offset left out
            _amr.check(L.amr_dsss_demod_device(pl.handle, d_x, F32, B, n + 9, d_out, cap + 3, d_len, d_sync, None, 0,
                                               None, acquire))
            pl.synchronize()
            out2, ln2 = d.get(d_out, np.zeros((B, cap + 3), np.uint8)), d.get(d_len, np.zeros(B, np.int64))
            assert np.array_equal(ln, ln2) and [out2[i, :ln[i]].tobytes() for i in range(B)] == [w[0] for w in want[:B]]
        # the argument contract, on a live plan
        args = (d_out, cap + 3, d_len, d_sync, None, 0, None, 1)
        assert L.amr_dsss_demod_device(pl.handle, d_x, F32, B + 1, n + 9, *args) == _amr.AMR_E_CAPACITY
        assert L.amr_dsss_demod_device(pl.handle, d_x, 7, B, n + 9, *args) == _amr.AMR_E_INVALID
        assert L.amr_dsss_demod_device(pl.handle, d_x, F32, B, n - 1, *args) == _amr.AMR_E_INVALID
        assert L.amr_dsss_demod_device(pl.handle, d_x, F32, B, n + 9, d_out, cap - 2, d_len, d_sync, None, 0, None, 1) == _amr.AMR_E_INVALID
        assert L.amr_dsss_demod_device(pl.handle, d_x, F32, B, n + 9, d_out, cap + 3, d_len, d_sync, d_soft, 8 * cap - 1,
                                       None, 1) == _amr.AMR_E_INVALID
        assert L.amr_dsss_demod_device(pl.handle, d_x, F32, 0, n + 9, *args) == _amr.AMR_OK


# ---- 5. transmit ----------------------------------------------------------------------------
TX_LENS = [0, 1, 2, 3, 5, 17, 64, 97]


@pytest.mark.parametrize("code,baud,carrier", [(None, 19200, 24000.0), (None, 9600, 12000.0), (None, 1200, 3000.0),
                                               (sp.CODE13, 9600, 12000.0), (sp.code64(), 9600, 24000.0)])
def test_modulate_batch_equals_the_restatement(code, baud, carrier):
    """Bit-equal: the sine is the host's table.  The natural length, shorter and longer; the padding exact
    zeros; the int16 samples those of the float32 ones."""
    import modem
    rng = np.random.default_rng(int(baud) + (0 if code is None else len(code)))
    datas = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in TX_LENS]
    L = sp.geometry(baud, carrier, code)[1]
    refs = [sp.modulate(d, baud, carrier, code) for d in datas]
    assert [r.size for r in refs] == [(81 + 8 * k) * L for k in TX_LENS]
    natural = max(r.size for r in refs)
    for n_out in (None, natural - 2 * L - 3, natural + 37):
        want = np.zeros((len(datas), natural if n_out is None else n_out), np.float32)
        for i, r in enumerate(refs):
            k = min(r.size, want.shape[1])
            want[i, :k] = r[:k]
        got, pcm = modem.modulate_batch("spread", datas, baud, carrier, n_out=n_out, pcm=True, code=code)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (baud, n_out)
        assert np.array_equal(pcm, (want * np.float32(32767)).astype(np.int16)), (baud, n_out)
        plain = modem.modulate_batch("spread", datas, baud, carrier, n_out=n_out, code=code)
        assert np.array_equal(plain.view(np.uint32), want.view(np.uint32))
    one = modem.spread_modulate(datas[5], baud, carrier, code)
    assert np.array_equal(one.view(np.uint32), refs[5].view(np.uint32))
    assert modem.modulate_batch("spread", [], baud, carrier, code=code).shape == (0, 0)


# ---- 6. loopback and the coded chain --------------------------------------------------------
def loop_configs():
    import ofdm_cases as oc
    return [(None, b, c) for b, c in oc.CONFIGS] + [(sp.CODE13, 9600, 12000.0), (sp.code64(), 9600, 12000.0)]


@pytest.mark.parametrize("sigma", [0.0, 0.5])
@pytest.mark.parametrize("code,baud,carrier", loop_configs())
def test_loopback_frames_parse(code, baud, carrier, sigma):
    """GPU modulator -> a delay per stream -> noise -> GPU acquisition and demodulator -> frame scan: every
    frame's payload comes back, CRC valid; clean, the offsets are the delays to the sample."""
    import modem
    from test_gpu_loopback import _frames, _payloads, _want_payload
    seed = int(baud) + (0 if code is None else len(code))
    rng = np.random.default_rng(seed)
    frames = _frames(3, 12, seed=seed)
    L = sp.geometry(baud, carrier, code)[1]
    w = modem.modulate_batch("spread", frames, baud, carrier, code=code)
    delays = rng.integers(0, L, len(frames))
    x = np.zeros((len(frames), w.shape[1] + 3 * L), np.float32)
    for i, t in enumerate(delays):
        x[i, t:t + w.shape[1]] = w[i]
    if sigma:
        x = x + rng.normal(0, sigma, x.shape).astype(np.float32)
    offs = modem.spread_acquire_batch(x, baud, carrier, code)
    if not sigma:
        assert list(offs) == list(delays)
    raws = modem.spread_demodulate_batch(x, baud, carrier, code)
    got = _payloads(raws)
    for i, fr in enumerate(frames):
        assert raws[i][:len(fr)] == fr and got[i] == [_want_payload(fr)], (baud, sigma, i)


def test_end_to_end_coded_chain():
    """encode_batch -> spread modulate -> a random delay per stream -> N(0, 2.8^2) -> acquisition and soft
    demodulation -> decode_soft_batch returns the messages.  9600 chips/s on a 12 kHz carrier, the default code,
    16 messages of 120 bytes, noise of 2.8 on a sine of amplitude 1 (about -12 dB per sample), seed 8.  The
    level is the largest of 2.0, 2.2 .. 3.4 at which this chain's restatement on the CPU (spread_cases.modulate
    -> demod_soft -> soft_cases.soft_decode_batch) returns all 16: at 2.0 .. 2.8 every offset is the delay to the
    sample, the sync word is found in all 16 streams and all 16 messages come back (0, 4, 8, 14, 15 of the 16
    hard codewords damaged); at 3.0 and 3.2 one stream loses the uncoded sync word, at 3.4 two.  The
    restatement runs here again, so the GPU's offsets and soft values are checked at this level too."""
    import fec
    import modem
    rng = np.random.default_rng(8)
    msgs = vc.messages(rng, [120] * 16)
    cws = fec.ConvolutionalEncoder().encode_batch(msgs)
    n_cw = len(cws[0])
    assert n_cw == 242 and cws == [vc.encode(m) for m in msgs]
    L = 160
    delays = rng.integers(0, L, 16)
    tx = modem.modulate_batch("spread", [b"FB" + c for c in cws], baud=9600, f0=12000.0)
    ref = np.stack([sp.modulate(b"FB" + c, 9600, 12000.0) for c in cws])
    assert np.array_equal(tx.view(np.uint32), ref.view(np.uint32))
    x = np.zeros((16, tx.shape[1] + 3 * L), np.float32)
    for i, t in enumerate(delays):
        x[i, t:t + tx.shape[1]] = tx[i]
    x = (x.astype(np.float64) + rng.normal(0, 2.8, x.shape)).astype(np.float32)
    outs, softs = modem.spread_demodulate_soft_batch(x, 9600, 12000.0)
    want = [sp.demod_soft(r, 9600, 12000.0) for r in x]
    assert [w[3] for w in want] == list(delays)
    assert list(modem.spread_acquire_batch(x, 9600, 12000.0)) == list(delays)
    assert outs == [w[0] for w in want] and all(np.array_equal(s, w[1]) for s, w in zip(softs, want))
    assert all(o[:2] == b"FB" and len(o) >= 2 + n_cw for o in outs)          # sync found in all
    assert sum(o[2:2 + n_cw] != c for o, c in zip(outs, cws)) >= 8             # and most hard codewords are damaged
    rows = [s[16:16 + 8 * n_cw] for s in softs]
    assert fec.ViterbiDecoder().decode_soft_batch(rows) == msgs


# ---- 7. the host layer spread shares with ofdm (sym_plan.h), at a small shape ----------------
# C = 4, spc = 3: L = 12.  n = 5 L + 3: five bits and a tail, 4 decided bits, no whole byte (out_cap 1);
# n = 21 L + 3: 20 decided bits, 2 bytes (out_cap 3).  The same cases as test_gpu_ofdm_acquire.py's section 4.
SMALL = (1000, 750.0, [1, 0, 1, 1], 3000)
SMALL_NS = [5 * 12 + 3, 21 * 12 + 3]
_small = {}


def small(dt, n):
    """(five rows of a wider array, poisoned behind n; the restatement's acquired and unacquired (bytes, soft,
    sync, o) of every row), computed once per module."""
    if (dt, n) not in _small:
        wide = np.random.default_rng(12 + n).normal(0, 0.3, (5, n + 4))
        wide = np.round(wide * 8000).astype(np.int16) if dt == "i16" else wide.astype(np.float32)
        wide[:, n:] = 32767 if dt == "i16" else np.nan
        x = wide[:, :n]
        _small[dt, n] = (x, [sp.demod_soft(r, *SMALL) for r in x], [sp.demod_soft(r, *SMALL, acquire_=False) for r in x])
    return _small[dt, n]


@pytest.mark.parametrize("n", SMALL_NS)
@pytest.mark.parametrize("dt", ["f32", "i16"])
def test_small_two_batches_of_wider_rows(dt, n):
    """Five streams through a plan of three (a full batch and a short one), x_stride > n: every host entry."""
    x, acq, plain = small(dt, n)
    assert sp.geometry(*SMALL)[:3] == (3, 12, 3) and x.strides[0] == (n + 4) * x.itemsize
    assert all(len(w[0]) == (n // 12 - 1) // 8 for w in plain)
    pl = plan_for(n, SMALL, 3)
    assert pl.out_cap == (n // 12 - 1) // 8 + 1
    for acquire, want in ((True, acq), (False, plain)):
        outs, syncs, softs, offs = pl.demod_host(x, soft=True, acquire=acquire)
        assert outs == [w[0] for w in want] and list(syncs) == [w[2] for w in want], (dt, acquire)
        assert list(offs) == [w[3] for w in want] and (acquire or not offs.any()), (dt, acquire)
        assert all(s.dtype == np.int8 and np.array_equal(s, w[1]) for s, w in zip(softs, want)), (dt, acquire)
        hard = pl.demod_host(x, acquire=acquire)
        assert hard[0] == outs and np.array_equal(hard[1], syncs) and hard[2] is None and np.array_equal(hard[3], offs)
    off, P = pl.acquire(x)
    woff, wP = want_acq(x, SMALL)
    assert np.array_equal(off, woff) and same_bits(P, wP) and list(off) == [w[3] for w in acq]
    assert same_bits(pl.symbols_at(x, off), want_Y(x, SMALL, off))
    assert same_bits(pl.symbols_at(x), want_Y(x, SMALL))


@pytest.mark.parametrize("n", SMALL_NS)
@pytest.mark.parametrize("dt", ["f32", "i16"])
def test_small_host_soft_rows_are_cut(dt, n):
    """soft_stride above 8 * out_cap with a sentinel in the slack, out_stride at its minimum: the row is cut at
    8 * out_len[i] and nothing behind it is written; the offsets are zeros when nothing is acquired."""
    import _amr
    x, acq, plain = small(dt, n)
    x = np.ascontiguousarray(x[:3])
    pl = plan_for(n, SMALL, 3)
    lib, cap = _amr.lib(), pl.out_cap
    stride = max(cap - 1, 1)
    for acquire, want in ((0, plain), (1, acq)):
        out, ln, sy = np.zeros((3, stride), np.uint8), np.zeros(3, np.int64), np.zeros(3, np.int64)
        soft, off = np.full((3, 8 * cap + 5), 77, np.int8), np.full(3, -99, np.int64)
        _amr.check(lib.amr_dsss_demod_host(pl.handle, _amr.ptr(x), _amr.DTYPES[x.dtype], 3, n, _amr.ptr(out), stride,
                                           _amr.ptr(ln), _amr.ptr(sy), _amr.ptr(soft), 8 * cap + 5, _amr.ptr(off), acquire))
        assert [out[i, :ln[i]].tobytes() for i in range(3)] == [w[0] for w in want[:3]]
        assert list(sy) == [w[2] for w in want[:3]] and list(ln) == [len(w[0]) for w in want[:3]]
        assert list(off) == [w[3] for w in want[:3]] and (acquire or list(off) == [0, 0, 0])
        for i in range(3):
            assert np.array_equal(soft[i, :8 * ln[i]], want[i][1]) and np.all(soft[i, 8 * ln[i]:] == 77), (acquire, i)
    assert n < 100 or min(ln) > 0                            # the longer capture has bytes to cut at


def test_small_empty_batch_and_fewer_than_two_bits():
    import _amr
    lib = _amr.lib()
    n = SMALL_NS[0]
    pl = plan_for(n, SMALL, 3)
    h, F32 = pl.handle, _amr.DTYPE_F32
    for acquire in (0, 1):
        assert lib.amr_dsss_demod_host(h, None, F32, 0, n, None, 1, None, None, None, 0, None, acquire) == _amr.AMR_OK
    assert lib.amr_dsss_acquire_host(h, None, F32, 0, n, None, None) == _amr.AMR_OK
    assert lib.amr_dsss_symbols_at_host(h, None, F32, 0, n, None, None) == _amr.AMR_OK
    rng = np.random.default_rng(3)
    for n in (3, 12 + 3):                                    # S = 0, 1
        x = rng.normal(0, 0.3, (5, n)).astype(np.float32)
        pl = plan_for(n, SMALL, 3)
        assert pl.out_cap == 1
        for acquire in (False, True):
            outs, syncs, softs, offs = pl.demod_host(x, soft=True, acquire=acquire)
            assert outs == [b""] * 5 and list(syncs) == [-1] * 5 and all(s.size == 0 for s in softs)
            assert list(offs) == [sp.acquire(r, *SMALL)[0] if acquire else 0 for r in x]


def test_small_scratch_bytes_are_the_estimates():
    import _amr
    n = SMALL_NS[0]
    x = small("f32", n)[0]
    lib = _amr.lib()
    plan_b, acq_b = lib.amr_dsss_plan_bytes_estimate(n, 3, 4, 3), lib.amr_dsss_acquire_bytes_estimate(n, 3, 4, 3)
    pl = plan_for(n, SMALL, 3)
    # Wc and T [L][2], cs [C], Y [ms][S][2], words [ms][1]: the plan before any call
    assert pl.scratch_bytes() == 2 * 12 * 16 + 4 * 8 + 3 * 5 * 16 + 3 * 4
    pl.demod_host(x, acquire=False)
    assert pl.scratch_bytes() == plan_b                      # + x [ms][n] doubles, out [ms][cap], len and sync [ms]
    assert plan_b == 2 * 12 * 16 + 4 * 8 + 3 * 5 * 16 + 3 * 4 + 3 * n * 8 + 3 * 1 + 2 * 3 * 8
    pl.demod_host(x)
    assert pl.scratch_bytes() == plan_b + acq_b              # + gq [ms][1][L], P [ms][L], off [ms]
    assert acq_b == 3 * 12 * 8 + 3 * 12 * 8 + 3 * 8
    pl.acquire(x)
    pl.demod_host(x, soft=True, acquire=False)
    assert pl.scratch_bytes() == plan_b + acq_b


def test_small_plans_come_and_go():
    """Create, demodulate twice on the host (the staging allocated, then reused), destroy; a few times over."""
    n = SMALL_NS[1]
    x, acq, plain = small("f32", n)
    for k in range(3):
        pl = plan_for(n, SMALL, 3)
        for _ in range(2):
            assert pl.demod_host(x, acquire=False)[0] == [w[0] for w in plain]
            assert pl.demod_host(x)[0] == [w[0] for w in acq]
        del pl
