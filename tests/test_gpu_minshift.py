"""minshift on the GPU: k_msk_corr, k_msk_lines, k_msk_acq_max,
k_msk_slice, k_msk_soft and the transmit kernels (msk_kernels.hip,
msk_acq_kernels.hip) with the plan / host layer around them, against the numpy
restatement in tests/minshift_cases.py: bit-equal throughout, the transmit
samples included."""
import numpy as np
import pytest

import minshift_cases as mc
import viterbi_cases as vc
from test_gpu_ofdm import same_bits
from test_gpu_viterbi import Dev

pytestmark = pytest.mark.gpu

# (L, cyc4): the smallest bit, an odd one, the default, an odd length that crosses a staging chunk of 32, two
# longer ones, and L = 300 whose line tables (2 L = 600 entries) do not fit LDS; cyc4 mod 4 = 2, 1, 3, 0, 2, 1, 1
GEOS = [(4, 2), (5, 5), (10, 7), (33, 32), (80, 10), (200, 201), (300, 77)]
WINDOWS = [1, 2, 63, 64, 65, 129]
STREAMS = [1, 2, 65]


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")
    assert "amr_msk_plan_create" in _amr.EXPORTS             # the restatement is only worth testing beside the product


def cfg(L, cyc4):
    """(baud, carrier, samp_rate) with exactly the geometry (L, cyc4)."""
    return mc.pair_of(L, cyc4)


def plan_for(n, c, B):
    import _amr
    baud, carrier, fs = c
    return _amr.MskPlan(n, baud, carrier, fs, max_streams=B)


def want_W(x, c, offs=None):
    offs = np.zeros(len(x), np.int64) if offs is None else offs
    return np.stack([mc.windows(r, o, *c) for r, o in zip(x, offs)])


def want_acq(x, c):
    got = [mc.acquire(r, *c) for r in x]
    return np.array([g[0] for g in got], np.int64), np.array([g[1] for g in got], np.complex128)


def test_the_geometries_cover_what_they_should():
    assert [L for L, _ in GEOS] == [4, 5, 10, 33, 80, 200, 300] and {c % 4 for _, c in GEOS} == {0, 1, 2, 3}
    assert {L % 4 for L, _ in GEOS} == {0, 1, 2}
    for L, cyc4 in GEOS:
        assert mc.geometry(*cfg(L, cyc4)) == (L, L // 2, cyc4)


# ---- 1. the window correlator alone ------------------------------------------------------------
# L = 7: L mod 4 = 3; L = 32 is exactly one staging chunk (33 in GEOS is one and a sample)
@pytest.mark.parametrize("L,cyc4", GEOS + [(7, 3), (32, 31)])
def test_corr_geometries_and_offsets(L, cyc4):
    """Offsets 0, 1, L - 1 and mixed per stream: the last window of a stream read from o > its slack is cut at n."""
    c = cfg(L, cyc4)
    rng = np.random.default_rng(100 * L + cyc4)
    n = 6 * L - L // 2 + 1                                   # Sw = 5 at any L; the last window ends a sample before n
    x = rng.standard_normal((4, n)).astype(np.float32)
    pl = plan_for(n, c, 4)
    got = pl.symbols_at(x)
    assert mc.n_windows(n, L) == 5 and got.shape == (4, 5) and same_bits(got, want_W(x, c))
    assert np.abs(got).max() > 0.5                           # not the zeros of a kernel that did not run
    for offs in ([0] * 4, [1] * 4, [L - 1] * 4, [L - 1, 0, 1, L // 2]):
        offs = np.array(offs, np.int64)
        assert same_bits(pl.symbols_at(x, offs), want_W(x, c, offs)), offs
    for bad in (-1, L):
        with pytest.raises(Exception):
            pl.symbols_at(x, np.array([0, bad, 0, 0], np.int64))


@pytest.mark.parametrize("S", WINDOWS)
@pytest.mark.parametrize("L,cyc4", [(10, 5), (5, 6)])
def test_corr_window_and_stream_counts(L, cyc4, S):
    """Flat window indices b*Sw + k cross wave edges inside and between streams; n at the least that holds S
    windows, a sample more, and a sample less than S + 1 would need."""
    c = cfg(L, cyc4)
    h = L // 2
    rng = np.random.default_rng(1000 * L + S)
    for B, r in zip(STREAMS, (0, 1, L - 1)):
        n = (S + 1) * L - h + r
        x = rng.standard_normal((B, n)).astype(np.float32)
        pl = plan_for(n, c, B)
        assert pl.S == S == mc.n_windows(n, L)
        got = pl.symbols_at(x)
        assert got.shape == (B, S) and same_bits(got, want_W(x, c)), (B, r)
        offs = rng.integers(0, L, B)
        assert same_bits(pl.symbols_at(x, offs), want_W(x, c, offs)), (B, r)
    # a plan larger than the batch, and a second call on it
    n = (S + 1) * L - h + 2
    pl = plan_for(n, c, 70)
    x = rng.standard_normal((3, n))
    for _ in range(2):
        got = pl.symbols_at(x)
        assert got.shape == (3, S) and same_bits(got, want_W(x, c))


def test_corr_no_window():
    c = cfg(10, 5)
    for n in (0, 4, 14):                                     # Sw = 0
        pl = plan_for(n, c, 2)
        assert pl.S == 0 and pl.symbols_at(np.ones((2, n), np.float32)).shape == (2, 0)


@pytest.mark.parametrize("dt", ["f32", "f64", "i16"])
def test_corr_dtypes_and_row_stride(dt):
    c = cfg(80, 10)
    n = 8 * 80 + 45
    rng = np.random.default_rng(3)
    wide = rng.standard_normal((5, n + 13))
    wide = np.round(wide * 9000).astype(np.int16) if dt == "i16" else wide.astype({"f32": np.float32, "f64": np.float64}[dt])
    x = wide[:, :n]                                          # rows of a wider array: x_stride = n + 13
    assert x.strides[0] == (n + 13) * x.itemsize and mc.n_windows(n, 80) == 8
    pl = plan_for(n, c, 8)
    offs = np.array([0, 79, 6, 5, 4], np.int64)              # 79 and 6 pass n in the last window: not the padding's samples
    assert same_bits(pl.symbols_at(x), want_W(x, c)) and same_bits(pl.symbols_at(x, offs), want_W(x, c, offs))
    assert same_bits(pl.symbols_at(np.ascontiguousarray(x), offs), want_W(x, c, offs))


def test_corr_special_samples():
    """+-inf, NaN, denormals and all zeros: float64 arithmetic has one answer for each (a NaN's sign aside)."""
    c = cfg(33, 32)
    n = 6 * 33
    rng = np.random.default_rng(4)
    x = rng.standard_normal((8, n))
    x[0] = 0.0
    x[1] = -0.0
    x[2, 60] = np.inf
    x[3, 100] = -np.inf
    x[3, 101] = np.inf
    x[4, 90] = np.nan
    x[5] = 5e-324 * rng.integers(-3, 4, n)
    x[6] *= 1e-310
    x[7] *= 1e300
    pl = plan_for(n, c, 8)
    offs = np.array([3, 0, 17, 32, 21, 2, 1, 0], np.int64)
    with np.errstate(all="ignore"):
        want = want_W(x, c)
        assert same_bits(pl.symbols_at(x), want) and same_bits(pl.symbols_at(x, offs), want_W(x, c, offs))
        assert not np.isfinite(want[2, 1].real) and np.isnan(want[4, 2].real) and not want[0].any()
        x32 = x.astype(np.float32)
        x32[5] = np.float32(1e-45) * rng.integers(-3, 4, n).astype(np.float32)     # float32 denormals
        assert np.any(x32[5] != 0)
        assert same_bits(pl.symbols_at(x32, offs), want_W(x32, c, offs))
    xi = np.zeros((2, n), np.int16)
    xi[1, ::7] = ([-32768, 32767] * 15)[:len(xi[1, ::7])]
    assert same_bits(pl.symbols_at(xi), want_W(xi, c))


# ---- 2. the bit timing alone ---------------------------------------------------------------------
def check_acquire(x, c, B=None):
    pl = plan_for(x.shape[1], c, B or len(x))
    off, q = pl.acquire(x)
    woff, wq = want_acq(x, c)
    assert q.shape == wq.shape and same_bits(q, wq)
    assert np.array_equal(off, woff), (off, woff)
    return off, q


@pytest.mark.parametrize("L,cyc4", GEOS)
def test_acquire_geometries(L, cyc4):
    """Noise, and a frame at a delay, found to the sample; the long frames span several segments."""
    c = cfg(L, cyc4)
    rng = np.random.default_rng(7 * L + cyc4)
    x = rng.standard_normal((3, 37 * L + L // 3)).astype(np.float32)
    off, q = check_acquire(x, c)
    assert np.all(q != 0)
    t = int(rng.integers(1, L))
    y = mc.delayed(b"FB" + bytes(3), t, *c[:2], samp_rate=c[2])[None, :]
    assert check_acquire(y, c)[0][0] == t


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193])
def test_acquire_lengths_around_a_segment(n):
    """None, a partial row, a whole row, one segment less a sample, one, one and a sample, two and a sample;
    1, 2 and 65 streams."""
    c = cfg(10, 7)
    rng = np.random.default_rng(n)
    for B in STREAMS:
        x = rng.standard_normal((B, n)).astype(np.float32)
        off, q = check_acquire(x, c)
        assert n > 0 or (not off.any() and not q.any())
    x = rng.standard_normal((3, n))                          # a plan larger than the batch, twice, float64
    pl = plan_for(n, c, 70)
    for _ in range(2):
        off, q = pl.acquire(x)
        woff, wq = want_acq(x, c)
        assert same_bits(q, wq) and np.array_equal(off, woff)


def test_acquire_long_bits_and_a_segment_edge():
    """L = 300 (tables from global memory) and L = 200 over segments whose first sample's table index differs."""
    rng = np.random.default_rng(77)
    for L, cyc4 in ((300, 77), (200, 201), (33, 32)):
        x = rng.standard_normal((2, 3 * 4096 + 17)).astype(np.float32)
        check_acquire(x, cfg(L, cyc4))


@pytest.mark.parametrize("dt", ["f32", "f64", "i16"])
def test_acquire_dtypes_row_stride_and_device_entry(dt):
    import _amr
    c = cfg(80, 10)
    n = 4096 + 711
    rng = np.random.default_rng(31)
    wide = rng.standard_normal((5, n + 13))
    wide = np.round(wide * 9000).astype(np.int16) if dt == "i16" else wide.astype({"f32": np.float32, "f64": np.float64}[dt])
    x = wide[:, :n]
    off, q = check_acquire(x, c, 8)
    pl = plan_for(n, c, 8)
    lib = _amr.lib()
    with Dev() as d:
        d_x, d_off, d_q = d.put(wide), d.put(np.zeros(5, np.int64)), d.put(np.zeros((5, 2)))
        _amr.check(lib.amr_msk_acquire_device(pl.handle, d_x, _amr.DTYPES[x.dtype], 5, n + 13, d_off, d_q))
        pl.synchronize()
        assert np.array_equal(d.get(d_off, np.zeros(5, np.int64)), off)
        assert same_bits(d.get(d_q, np.zeros((5, 2))), q)
        _amr.check(lib.amr_msk_acquire_device(pl.handle, d_x, _amr.DTYPES[x.dtype], 2, n + 13, d_off, None))   # q optional
        pl.synchronize()
        assert lib.amr_msk_acquire_device(pl.handle, d_x, _amr.DTYPES[x.dtype], 9, n + 13, d_off, None) == _amr.AMR_E_CAPACITY
        assert lib.amr_msk_acquire_device(pl.handle, d_x, 7, 5, n + 13, d_off, None) == _amr.AMR_E_INVALID
        assert lib.amr_msk_acquire_device(pl.handle, d_x, _amr.DTYPES[x.dtype], 5, n - 1, d_off, None) == _amr.AMR_E_INVALID


def test_acquire_zeros_nan_and_infinities():
    c = cfg(10, 7)
    rng = np.random.default_rng(32)
    n = 2 * 4096 + 300
    x = rng.standard_normal((6, n)).astype(np.float32)
    x[0] = 0.0                                               # all zeros: q = 0, o = 0
    x[1, 0] = np.nan                                         # a NaN anywhere: q is NaN, 0 is kept
    x[2, 4096 + 5] = np.nan
    x[3, n - 1] = np.inf                                     # inf * inf * table: inf or NaN in both lines
    x[4, 17] = -np.inf
    x[5] = 0.0
    x[5, 8192 + 123] = -1.5                                  # one sample alone, in the short last segment
    with np.errstate(all="ignore"):
        off, q = check_acquire(x, c)
    assert off[0] == 0 and q[0] == 0
    assert list(off[1:5]) == [0, 0, 0, 0] and np.all(np.isnan(q[1:5].real) | np.isnan(q[1:5].imag))
    assert q[5] != 0


def test_offset_on_crafted_sums():
    """amr_msk_offset_host: an exact tie of P (the first index wins, across lanes too), a NaN q, q = 0."""
    import _amr
    nan = np.nan
    for L, cyc4 in ((10, 7), (200, 201)):
        baud, carrier, fs = cfg(L, cyc4)
        cs = [(1.0, 0.0, 1.0, 0.0),                          # q = 1: P[d] = cos(2 pi d / L), greatest at 0
              (1.0, 0.0, -1.0, 0.0),                         # q = -1: greatest at L / 2
              (1.0, 0.0, 0.0, 1.0),                          # q = i: P[d] = -sin, the table's own tie rule decides
              (1.0, 0.0, 0.0, -1.0),
              (0.0, 0.0, 3.0, 4.0),                          # c0 = 0: q = 0, every P is 0: an exact tie of all L, 0 wins
              (-0.0, 0.0, 3.0, -4.0),
              (1.0, 2.0, nan, 0.0), (nan, nan, 1.0, 1.0),    # a NaN q
              (0.3, -0.7, 1.1, 0.9), (2.0 ** 600, 0.0, 2.0 ** 600, 0.0), (np.inf, 0.0, 1.0, 0.0)]
        c = np.array(cs)
        with np.errstate(all="ignore"):
            off, q = _amr.msk_offset(c, baud, carrier, fs)
            want = [mc.offset_of(complex(a, b), complex(e, f), baud, carrier, fs) for a, b, e, f in cs]
        assert list(off) == [w[0] for w in want], (L, off)
        assert same_bits(q, np.array([w[1] for w in want], np.complex128))
        assert off[0] == 0 and off[1] == L // 2 and off[4] == 0 and off[5] == 0 and off[6] == 0 and off[7] == 0
    # an exact two-way tie that is not at 0: q = -1 at odd L has P[(L - 1) / 2] and P[(L + 1) / 2] equal up to the
    # table's rounding; whichever the restatement's sequential rule takes, the wave's parallel search takes
    for L, cyc4 in ((5, 5), (33, 32)):
        baud, carrier, fs = cfg(L, cyc4)
        off, q = _amr.msk_offset(np.array([[1.0, 0.0, -1.0, 0.0]]), baud, carrier, fs)
        assert off[0] == mc.offset_of(1 + 0j, -1 + 0j, baud, carrier, fs)[0] and off[0] in ((L - 1) // 2, (L + 1) // 2)
    # R at L = 4 is (1, 0), (0, 1), (-1, 0), (0, -1) up to cos(pi / 2)'s 6e-17: q = 1 + i ties P[0] = 1 with
    # P[3] = 1 exactly if the table's zeros were exact; the restatement says which
    baud, carrier, fs = cfg(4, 2)
    off, q = _amr.msk_offset(np.array([[1.0, 0.0, 1.0, 1.0], [1.0, 0.0, 1.0, -1.0]]), baud, carrier, fs)
    assert list(off) == [mc.offset_of(1 + 0j, 1 + 1j, baud, carrier, fs)[0], mc.offset_of(1 + 0j, 1 - 1j, baud, carrier, fs)[0]]


# ---- 3. the slicer and the soft stage alone ---------------------------------------------------
def want_bits(W, cyc4):
    return np.stack([mc.slice_bits(w, cyc4) for w in W])


def want_soft(W, cyc4):
    return np.stack([mc.soft(w, cyc4) for w in W])


def test_slice_and_soft_stage_sizes():
    """1 .. 300 products per stream: a word's 32 bits, a wave's two words, k_msk_soft's 256-thread block; the
    four quarter-turns."""
    import _amr
    rng = np.random.default_rng(20)
    for k, nd in enumerate((1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300)):
        for B in (1, 3, 65):
            cyc4 = 4 + (k + B) % 4
            W = rng.standard_normal((B, nd + 1)) + 1j * rng.standard_normal((B, nd + 1))
            bits, soft = _amr.msk_slice(W, cyc4), _amr.msk_soft(W, cyc4)
            assert bits.shape == (B, nd) and np.array_equal(bits, want_bits(W, cyc4)), (nd, B)
            assert soft.dtype == np.int8 and np.array_equal(soft, want_soft(W, cyc4)), (nd, B)
            assert np.array_equal(soft > 0, bits.astype(bool))                       # the sign is the hard bit
    assert _amr.msk_slice(np.ones((3, 1), np.complex128), 5).shape == (3, 0)         # Sw = 1: nothing
    assert _amr.msk_soft(np.ones((3, 1), np.complex128), 5).shape == (3, 0)


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_special_products(rot):
    """Exact zeros of either sign, a component an ulp to each side of 0, NaN, inf and 2^+-500 in either component,
    under each quarter-turn: D.imag of +0.0, -0.0 and NaN each give bit 0."""
    import _amr
    tiny = 5e-324
    v = [0.0, -0.0, tiny, -tiny, 2.0 ** -500, -2.0 ** -500, 2.0 ** 500, -2.0 ** 500, np.inf, -np.inf, np.nan, 1.0, -1.0,
         np.nextafter(1.0, 2.0), -np.nextafter(1.0, 0.0)]
    d = np.array([complex(a, b) for a in v for b in v])
    # window 0 is 1, so the product of (1, d) is d itself wherever d is finite: the cases decide what they say
    W = np.ascontiguousarray(np.stack([np.ones(d.size), d], axis=1))                 # [streams][Sw = 2]
    cyc4 = 8 + rot
    with np.errstate(all="ignore"):
        D = np.concatenate([mc.products(w, cyc4) for w in W])
        fin = np.isfinite(d.real) & np.isfinite(d.imag)
        assert np.array_equal(D[fin], (d * (-1j) ** rot)[fin]) and fin.sum() > 100
        bits, soft = _amr.msk_slice(W, cyc4), _amr.msk_soft(W, cyc4)
        assert np.array_equal(bits, want_bits(W, cyc4)) and np.array_equal(soft, want_soft(W, cyc4))
        assert not np.any(soft == 0) and not np.any(soft == -128)
        assert np.array_equal(bits[:, 0] == 1, D.imag > 0)
        zero = D.imag == 0
        assert np.signbit(D.imag[zero]).any() and not np.signbit(D.imag[zero]).all()   # zeros of both signs are there
        assert not bits[zero].any() and not bits[np.isnan(D.imag)].any() and np.isnan(D.imag).sum() > 10
        # the same values along one stream's time axis: windows 1, d, 1, d' ... give d, conj(d), d' ...
        Z = np.ones((1, 2 * d.size), np.complex128)
        Z[0, 1::2] = d
        assert np.array_equal(_amr.msk_slice(Z, cyc4), want_bits(Z, cyc4))
        assert np.array_equal(_amr.msk_soft(Z, cyc4), want_soft(Z, cyc4))


# ---- 4. full demodulation -------------------------------------------------------------------
CASES = {"b96": (9600, 12000.0, 96000), "b12": (1200, 3000.0, 96000)}
SIGMA = {"b96": 0.15, "b12": 0.5}
B_MAX = 67
SHORT = 5                 # streams of the float64 and int16 batches (the restatement's time)
_cases = {}


def make_batch(name, dt):
    """[B][n] streams at random delays under noise: frames whose sync word sits 0 .. 7 bits into a byte, and
    noise alone (no sync word)."""
    baud, carrier, fs = CASES[name]
    rng = np.random.default_rng(len(name) + int(baud))
    L = mc.geometry(baud, carrier, fs)[0]
    room = 6
    n = (82 + 8 * (room + 3)) * L + 2 * L + 17
    rows = []
    for i in range(B_MAX if dt == "f32" else SHORT):
        x = np.zeros(n, np.float32)
        if i % 3 != 2:
            shift = (i // 3) % 8
            body = b"FB" + rng.integers(0, 256, room, dtype=np.uint8).tobytes()
            bits = np.concatenate([np.zeros(shift, np.uint8), np.unpackbits(np.frombuffer(body, np.uint8)),
                                   np.zeros(8 - shift, np.uint8)])
            w = mc.modulate(np.packbits(bits).tobytes(), baud, carrier, fs)
            t = int(rng.integers(0, L))
            x[t:t + w.size] = w
        rows.append(x + rng.normal(0, SIGMA[name], n))
    x = np.stack(rows)
    if dt == "i16":
        return np.round(np.clip(x, -3.9, 3.9) * 8000).astype(np.int16)
    return x.astype(np.float32 if dt == "f32" else np.float64)


def case(name, dt):
    """(x, acquired [(bytes, soft, sync, o)], unacquired the same) from the restatement, computed once per module."""
    if (name, dt) not in _cases:
        x = make_batch(name, dt)
        c = CASES[name]
        _cases[name, dt] = (x, [mc.demod_soft(r, *c) for r in x], [mc.demod_soft(r, *c, acquire_=False) for r in x])
    return _cases[name, dt]


def test_the_cases_hold_what_they_should():
    for name in CASES:
        x, acq, plain = case(name, "f32")
        syncs = np.array([w[2] for w in acq])
        assert np.sum(syncs >= 0) >= 35 and np.sum(syncs < 0) >= 15 and all(len(w[0]) > 0 for w in acq), (name, syncs)
        assert len({int(s) % 8 for s in syncs if s >= 0}) == 8                   # every alignment of the sync word
        assert len({w[3] for w in acq}) >= (8 if name == "b96" else 20)          # the delays differ
        assert sum(a[0] != p[0] for a, p in zip(acq, plain)) > 20                # and the bit timing matters
        assert all(mc.demod(r, *CASES[name])[:2] == (w[0], w[2]) for r, w in zip(x[:3], acq))


@pytest.mark.parametrize("acquire", [True, False])
@pytest.mark.parametrize("dt", ["f32", "f64", "i16"])
@pytest.mark.parametrize("name", list(CASES))
def test_demod_equals_the_restatement(name, dt, acquire):
    import _amr
    baud, carrier, fs = CASES[name]
    x, acq, plain = case(name, dt)
    want = acq if acquire else plain
    n = x.shape[1]
    for B in sorted({1, 3, len(x)}):
        pl = _amr.MskPlan(n, baud, carrier, fs, max_streams=B)
        assert pl.out_cap == (mc.n_windows(n, pl.L) - 1) // 8 + 1
        outs, sync, softs, offs = pl.demod_host(x[:B], soft=True, acquire=acquire)
        assert outs == [w[0] for w in want[:B]], (name, dt, B)
        assert list(sync) == [w[2] for w in want[:B]] and list(offs) == [w[3] for w in want[:B]], (name, dt, B)
        for i, w in enumerate(want[:B]):
            assert softs[i].dtype == np.int8 and np.array_equal(softs[i], w[1]), (name, dt, B, i)
            assert np.packbits(softs[i] > 0).tobytes() == outs[i]
        hard = pl.demod_host(x[:B], acquire=acquire)
        assert hard[0] == outs and np.array_equal(hard[1], sync) and hard[2] is None and np.array_equal(hard[3], offs)
    # more streams than the plan holds: the host layer cuts the batch
    pl = _amr.MskPlan(n, baud, carrier, fs, max_streams=4)
    assert pl.demod_host(x, acquire=acquire)[0] == [w[0] for w in want]


def test_modem_functions_plan_cache_and_timings():
    import _amr
    import modem
    baud, carrier, fs = CASES["b96"]
    x, acq, plain = case("b96", "f32")
    n = x.shape[1]
    assert modem.minshift_demodulate_batch(x[:9], baud, carrier) == [w[0] for w in acq[:9]]
    assert modem.minshift_demodulate_batch(x[:9], baud, carrier, acquire=False) == [w[0] for w in plain[:9]]
    assert modem.minshift_demodulate(x[1], baud, carrier) == acq[1][0]
    assert list(modem.minshift_acquire_batch(x[:9], baud, carrier)) == [w[3] for w in acq[:9]]
    assert modem.minshift_acquire(x[4], baud, carrier) == acq[4][3]
    x16 = x[1].astype(np.float16)                            # anything but float32 / float64 / int16 goes as float64
    assert modem.minshift_demodulate(x16, baud, carrier) == mc.demod(x16, baud, carrier)[0]
    so, sv = modem.minshift_demodulate_soft_batch(x[:9], baud, carrier)
    assert so == [w[0] for w in acq[:9]] and all(np.array_equal(a, w[1]) for a, w in zip(sv, acq))
    d1, s1 = modem.minshift_demodulate_soft(x[4], baud, carrier, acquire=False)
    assert d1 == plain[4][0] and np.array_equal(s1, plain[4][1])
    # the cache counts the bit-timing buffers once a plan acquires
    pl = _amr.get_msk_plan(n, baud, carrier, None, fs, 9)
    assert pl is _amr.get_msk_plan(n, baud, carrier, None, fs, 3) and pl.max_streams == 16
    assert pl is not _amr.get_msk_plan(n, baud, 14400.0, None, fs, 3)
    lib = _amr.lib()
    total = lib.amr_msk_plan_bytes_estimate(n, 10, 16) + lib.amr_msk_acquire_bytes_estimate(n, 10, 16)
    assert lib.amr_msk_acquire_bytes_estimate(n, 10, 16) < pl.scratch_bytes() <= total
    fresh = _amr.MskPlan(n, baud, carrier, fs, max_streams=4)
    before = fresh.scratch_bytes()
    assert before == 6 * 10 * 16 + 4 * fresh.S * 16 + 4 * ((fresh.S - 1 + 31) // 32) * 4   # U, E0, E1, R, W, words
    fresh.demod_host(x[:4], acquire=False)
    staged = fresh.scratch_bytes()
    assert staged == lib.amr_msk_plan_bytes_estimate(n, 10, 4)
    fresh.acquire(x[:4])
    assert before < staged and fresh.scratch_bytes() == staged + lib.amr_msk_acquire_bytes_estimate(n, 10, 4)
    pl.enable_timing()
    pl.demod_host(x[:9], acquire=False)
    t = pl.timings()
    assert set(t) == {"despread", "slice", "sync_pack", "launch"} and all(v >= 0 for v in t.values())
    pl.demod_host(x[:9], soft=True)
    t = pl.timings()
    assert set(t) == set(_amr.TD_SLOTS) and t["launch"] >= max(t["acquire"], t["despread"], t["slice"], t["sync_pack"])
    pl.enable_timing(False)
    # the alias stays the reference's FSK with tone spacing baud
    assert np.array_equal(modem.msk_modulate(b"FBPC", 9600, 12000.0), modem.fsk_modulate(b"FBPC", 9600, 12000.0, 21600.0))


def test_fewer_than_two_windows_is_empty():
    import _amr
    import modem
    rng = np.random.default_rng(1)
    for n in (0, 14, 15, 24):                                # Sw = 0, 0, 1, 1 at L = 10
        x = rng.normal(0, 0.3, (3, n)).astype(np.float32)
        pl = _amr.MskPlan(n, 9600, 12000.0, max_streams=3)
        assert pl.out_cap == 1
        for acquire in (False, True):
            outs, sync, softs, offs = pl.demod_host(x, soft=True, acquire=acquire)
            assert outs == [b""] * 3 and list(sync) == [-1] * 3 and all(s.size == 0 for s in softs)
            assert list(offs) == [mc.acquire(r, 9600, 12000.0)[0] if acquire else 0 for r in x]
    assert modem.minshift_demodulate(np.zeros(20, np.float32), 9600, 12000.0) == b""
    lib = _amr.lib()
    pl = _amr.MskPlan(100, 9600, 12000.0, max_streams=3)
    for acquire in (0, 1):                                   # an empty batch
        assert lib.amr_msk_demod_host(pl.handle, None, 0, 0, 100, None, 1, None, None, None, 0, None, acquire) == _amr.AMR_OK
    assert lib.amr_msk_acquire_host(pl.handle, None, 0, 0, 100, None, None) == _amr.AMR_OK
    assert lib.amr_msk_symbols_at_host(pl.handle, None, 0, 0, 100, None, None) == _amr.AMR_OK


def test_device_entries():
    """amr_msk_demod_device on the caller's buffers: wider rows, the soft rows pre-filled, soft and offset
    optional, acquired and not: the same bytes, values and offsets as the host entry."""
    import _amr
    baud, carrier, fs = CASES["b96"]
    x, acq, plain = case("b96", "f32")
    n = x.shape[1]
    B = 65
    L = _amr.lib()
    pl = _amr.MskPlan(n, baud, carrier, fs, max_streams=B)
    cap = pl.out_cap
    xw = np.zeros((B, n + 9), np.float32)
    xw[:, :n] = x[:B]
    xw[:, n:] = np.nan                                       # the padding is never read
    F32 = _amr.DTYPE_F32
    with Dev() as d:
        d_x = d.put(xw)
        d_out, d_len, d_sync = d.put(np.zeros((B, cap + 3), np.uint8)), d.put(np.zeros(B, np.int64)), d.put(np.zeros(B, np.int64))
        d_off = d.put(np.full(B, -5, np.int64))
        for acquire, want in ((1, acq), (0, plain)):
            d_soft = d.put(np.full((B, 8 * cap + 5), 77, np.int8))
            _amr.check(L.amr_msk_demod_device(pl.handle, d_x, F32, B, n + 9, d_out, cap + 3, d_len, d_sync, d_soft,
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
            _amr.check(L.amr_msk_demod_device(pl.handle, d_x, F32, B, n + 9, d_out, cap + 3, d_len, d_sync, None, 0,
                                              None, acquire))
            pl.synchronize()
            out2, ln2 = d.get(d_out, np.zeros((B, cap + 3), np.uint8)), d.get(d_len, np.zeros(B, np.int64))
            assert np.array_equal(ln, ln2) and [out2[i, :ln[i]].tobytes() for i in range(B)] == [w[0] for w in want[:B]]
        # the argument contract, on a live plan
        args = (d_out, cap + 3, d_len, d_sync, None, 0, None, 1)
        assert L.amr_msk_demod_device(pl.handle, d_x, F32, B + 1, n + 9, *args) == _amr.AMR_E_CAPACITY
        assert L.amr_msk_demod_device(pl.handle, d_x, 7, B, n + 9, *args) == _amr.AMR_E_INVALID
        assert L.amr_msk_demod_device(pl.handle, d_x, F32, B, n - 1, *args) == _amr.AMR_E_INVALID
        assert L.amr_msk_demod_device(pl.handle, d_x, F32, B, n + 9, d_out, cap - 2, d_len, d_sync, None, 0, None, 1) == _amr.AMR_E_INVALID
        assert L.amr_msk_demod_device(pl.handle, d_x, F32, B, n + 9, d_out, cap + 3, d_len, d_sync, d_soft, 8 * cap - 1,
                                      None, 1) == _amr.AMR_E_INVALID
        assert L.amr_msk_demod_device(pl.handle, d_x, F32, 0, n + 9, *args) == _amr.AMR_OK


# ---- 5. transmit ----------------------------------------------------------------------------
TX_LENS = [0, 1, 2, 3, 5, 17, 64, 97]


@pytest.mark.parametrize("baud,carrier,fs", [(19200, 24000.0, 96000), (9600, 12000.0, 96000), (1200, 3000.0, 96000),
                                             mc.pair_of(4, 6), mc.pair_of(33, 32), mc.pair_of(7, 3)])
def test_modulate_batch_equals_the_restatement(baud, carrier, fs):
    """Bit-equal: the sine is the host's table.  The natural length, shorter and longer; the padding exact
    zeros; the int16 samples those of the float32 ones."""
    import modem
    rng = np.random.default_rng(int(baud) + int(carrier))
    datas = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in TX_LENS]
    L = mc.geometry(baud, carrier, fs)[0]
    refs = [mc.modulate(d, baud, carrier, fs) for d in datas]
    assert [r.size for r in refs] == [(82 + 8 * k) * L for k in TX_LENS]
    natural = max(r.size for r in refs)
    for n_out in (None, natural - 2 * L - 3, natural + 37):
        want = np.zeros((len(datas), natural if n_out is None else n_out), np.float32)
        for i, r in enumerate(refs):
            k = min(r.size, want.shape[1])
            want[i, :k] = r[:k]
        got, pcm = modem.modulate_batch("minshift", datas, baud, carrier, samp_rate=fs, n_out=n_out, pcm=True)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (baud, n_out)
        assert pcm.dtype == np.int16 and np.array_equal(pcm, (want * np.float32(32767)).astype(np.int16)), (baud, n_out)
        plain = modem.modulate_batch("minshift", datas, baud, carrier, samp_rate=fs, n_out=n_out)
        assert np.array_equal(plain.view(np.uint32), want.view(np.uint32))
    one = modem.minshift_modulate(datas[5], baud, carrier, fs)
    assert np.array_equal(one.view(np.uint32), refs[5].view(np.uint32))
    assert modem.modulate_batch("minshift", [], baud, carrier, samp_rate=fs).shape == (0, 0)


# ---- 6. loopback and the coded chain --------------------------------------------------------
def loop_configs():
    import ofdm_cases as oc
    return list(oc.CONFIGS)


@pytest.mark.parametrize("baud,carrier", loop_configs())
def test_loopback_frames_parse(baud, carrier):
    """GPU modulator -> a random delay per stream -> GPU bit timing and demodulator -> frame scan: every frame's
    payload comes back, CRC valid, and the offsets are the delays to the sample; then the same under N(0, 0.1^2),
    where the payloads still come back."""
    import modem
    from test_gpu_loopback import _frames, _payloads, _want_payload
    seed = int(baud)
    rng = np.random.default_rng(seed)
    frames = _frames(3, 12, seed=seed)
    L = mc.geometry(baud, carrier)[0]
    w = modem.modulate_batch("minshift", frames, baud, carrier)
    delays = rng.integers(0, L, len(frames))
    x = np.zeros((len(frames), w.shape[1] + 3 * L), np.float32)
    for i, t in enumerate(delays):
        x[i, t:t + w.shape[1]] = w[i]
    for sigma in (0.0, 0.1):
        y = x + rng.normal(0, sigma, x.shape).astype(np.float32) if sigma else x
        offs = modem.minshift_acquire_batch(y, baud, carrier)
        if not sigma:
            assert list(offs) == list(delays)
        raws = modem.minshift_demodulate_batch(y, baud, carrier)
        assert raws == [mc.demod(r, baud, carrier)[0] for r in y]
        got = _payloads(raws)
        for i, fr in enumerate(frames):
            assert raws[i][:len(fr)] == fr and got[i] == [_want_payload(fr)], (baud, sigma, i)


def test_end_to_end_coded_chain():
    """encode_batch -> minshift modulate -> a random delay per stream -> N(0, 0.5^2) -> bit timing and soft
    demodulation -> decode_soft_batch returns the messages.  9600 Bd on a 12 kHz carrier (10 samples per bit), 16
    messages of 120 bytes, seed 8.  The level is the largest of the ladder 0.3, 0.4 .. 1.2 at which this chain's
    restatement on the CPU (minshift_cases.modulate -> demod_soft -> soft_cases.soft_decode_batch) returns all
    16: at 0.3, 0.4 and 0.5 every offset is the delay to the sample, the sync word is found in all 16 streams and
    all 16 messages come back (9, 16 and 16 of the 16 hard codewords damaged); from 0.6 on streams lose the
    uncoded sync word (13, 11, 10, 7, 5, 3 and 1 of 16 keep it at 0.6 .. 1.2), though every offset is still
    exact.  The restatement runs here again, so the GPU's offsets and soft values are checked at this level too."""
    import fec
    import modem
    rng = np.random.default_rng(8)
    msgs = vc.messages(rng, [120] * 16)
    cws = fec.ConvolutionalEncoder().encode_batch(msgs)
    n_cw = len(cws[0])
    assert n_cw == 242 and cws == [vc.encode(m) for m in msgs]
    L = 10
    delays = rng.integers(0, L, 16)
    tx = modem.modulate_batch("minshift", [b"FB" + c for c in cws], baud=9600, f0=12000.0)
    ref = np.stack([mc.modulate(b"FB" + c, 9600, 12000.0) for c in cws])
    assert np.array_equal(tx.view(np.uint32), ref.view(np.uint32))
    x = np.zeros((16, tx.shape[1] + 3 * L), np.float32)
    for i, t in enumerate(delays):
        x[i, t:t + tx.shape[1]] = tx[i]
    x = (x.astype(np.float64) + rng.normal(0, 0.5, x.shape)).astype(np.float32)
    outs, softs = modem.minshift_demodulate_soft_batch(x, 9600, 12000.0)
    want = [mc.demod_soft(r, 9600, 12000.0) for r in x]
    assert [w[3] for w in want] == list(delays)
    assert list(modem.minshift_acquire_batch(x, 9600, 12000.0)) == list(delays)
    assert outs == [w[0] for w in want] and all(np.array_equal(s, w[1]) for s, w in zip(softs, want))
    assert all(o[:2] == b"FB" and len(o) >= 2 + n_cw for o in outs)          # sync found in all
    assert sum(o[2:2 + n_cw] != c for o, c in zip(outs, cws)) >= 8             # and most hard codewords are damaged
    rows = [s[16:16 + 8 * n_cw] for s in softs]
    assert fec.ViterbiDecoder().decode_soft_batch(rows) == msgs
