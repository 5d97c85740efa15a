"""tone8 on the GPU: k_tone8_acq, k_tone8_peak, k_tone8_acq_max,
k_tone8_dft, k_tone8_slice, k_tone8_soft and the transmit kernels
(tone8_kernels.hip, tone8_acq_kernels.hip) with the plan / host layer around
them, against the numpy restatement in tests/tone8_cases.py: bit-equal
throughout, the transmit samples included."""
import numpy as np
import pytest

import tone8_cases as tc
import viterbi_cases as vc
from test_gpu_ofdm import same_bits
from test_gpu_viterbi import Dev

pytestmark = pytest.mark.gpu

# (L, c2, G): the smallest symbol; no search; the 1200 Bd default on 3000 Hz with its widest search; the default
# search; L = 1920 whose table (3840 entries) does not fit LDS; the widest search (47 lines, a chunk of 13)
GEOS = [(24, 4, 1), (40, 10, 0), (80, 5, 3), (160, 40, 6), (1920, 40, 6), (80, 36, 16)]
STREAMS = [1, 2, 65]


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")
    assert "amr_tone8_plan_create" in _amr.EXPORTS           # the restatement is only worth testing beside the product


def cfg(L, c2):
    """(baud, carrier, samp_rate) with exactly the geometry (L, c2)."""
    return tc.pair_of(L, c2)


def plan_for(n, c, G, B):
    import _amr
    baud, carrier, fs = c
    return _amr.Tone8Plan(n, baud, carrier, fs, G, max_streams=B)


def want_acq(x, c, G):
    with np.errstate(all="ignore"):
        got = [tc.acquire(r, *c, G) for r in x]
    return (np.array([g[0] for g in got], np.int64), np.array([g[1] for g in got], np.int64),
            np.array([g[2] for g in got], np.float64))


def check_acquire(x, c, G, B=None):
    pl = plan_for(x.shape[1], c, G, B or len(x))
    start, shift, score = pl.acquire(x)
    ws, wg, wv = want_acq(x, c, G)
    assert np.array_equal(start, ws) and np.array_equal(shift, wg), (start, ws, shift, wg)
    assert same_bits(score, wv)
    return start, shift, score


def test_the_geometries_cover_what_they_should():
    import _amr
    for L, c2, G in GEOS:
        assert tc.geometry(*cfg(L, c2), G) == (L, L // 8, c2, G)
    assert [_amr.tone8_chunk(G) for _, _, G in GEOS] == [134, 159, 98, 64, 64, 13]
    assert sum(2 * L > 512 for L, _, _ in GEOS) == 1


# ---- 1. acquisition alone --------------------------------------------------------------------
@pytest.mark.parametrize("L,c2,G", GEOS)
def test_acquire_chunk_edges(L, c2, G):
    """nj = -1, 0, 1, C - 1, C, C + 1 and 2 C + 1 start slots, n never a multiple of T; 1, 2 and 65 streams in
    turn; noise, with a frame's Costas block in the first, a middle and the last start slot of some streams."""
    import _amr
    c = cfg(L, c2)
    T, C = L // 8, _amr.tone8_chunk(G)
    rng = np.random.default_rng(100 * L + c2)
    block = tc.modulate(b"", *c)                             # the Costas block alone: 7 L samples
    for k, nj in enumerate((-1, 0, 1, C - 1, C, C + 1, 2 * C + 1)):
        n = (nj + 55) * T + 1 + k % (T - 1)
        B = STREAMS[k % 3]
        x = rng.normal(0, 0.2, (B, n)).astype(np.float32)
        slots = [0, nj // 2, nj - 1] if nj > 0 else []
        for b, j in enumerate(slots[:B]):
            x[b, j * T:j * T + block.size] += block[:n - j * T]
        start, shift, score = check_acquire(x, c, G)
        assert n % T and n // T - 55 == nj
        if nj <= 0:
            assert not start.any() and not shift.any() and not score.any()
        for b, j in enumerate(slots[:B]):
            assert (start[b], shift[b]) == (j * T, 0), (nj, b)


def test_acquire_many_chunks_and_a_plan_larger_than_the_batch():
    """65 streams over 7 chunks at the default search, frames at random slots with the sender off the grid line;
    a second call on the same plan."""
    L, c2, G = 160, 40, 6
    c = cfg(L, c2)
    T = L // 8
    rng = np.random.default_rng(5)
    n = 400 * T + 7
    x = rng.normal(0, 0.3, (65, n)).astype(np.float32)
    want = []
    for b in range(65):
        t = int(rng.integers(0, (400 - 56) * T))
        off = int(rng.integers(-G, G + 1))
        w = tc.modulate(b"FB", c[0], c[1] + off * c[0] / 2, c[2])
        x[b, t:t + w.size] += w[:n - t]
        want.append((t, off))
    start, shift, _ = check_acquire(x, c, G, 70)
    assert all(abs(s - t) <= T and g == off for s, g, (t, off) in zip(start, shift, want))
    pl = plan_for(n, c, G, 70)
    for _ in range(2):
        got = pl.acquire(x[:3])
        ws, wg, wv = want_acq(x[:3], c, G)
        assert np.array_equal(got[0], ws) and np.array_equal(got[1], wg) and same_bits(got[2], wv)


@pytest.mark.parametrize("dt", ["f32", "f64", "i16"])
def test_acquire_dtypes_row_stride_and_device_entry(dt):
    import _amr
    L, c2, G = 80, 5, 3
    c = cfg(L, c2)
    n = 230 * 10 + 3
    rng = np.random.default_rng(31)
    wide = rng.standard_normal((5, n + 13))
    wide = np.round(wide * 9000).astype(np.int16) if dt == "i16" else wide.astype({"f32": np.float32, "f64": np.float64}[dt])
    x = wide[:, :n]                                          # rows of a wider array: x_stride = n + 13
    start, shift, score = check_acquire(x, c, G, 8)
    pl = plan_for(n, c, G, 8)
    lib = _amr.lib()
    with Dev() as d:
        d_x, d_st, d_sh, d_sc = d.put(wide), d.put(np.zeros(5, np.int64)), d.put(np.zeros(5, np.int64)), d.put(np.zeros(5))
        _amr.check(lib.amr_tone8_acquire_device(pl.handle, d_x, _amr.DTYPES[x.dtype], 5, n + 13, d_st, d_sh, d_sc))
        pl.synchronize()
        assert np.array_equal(d.get(d_st, np.zeros(5, np.int64)), start)
        assert np.array_equal(d.get(d_sh, np.zeros(5, np.int64)), shift)
        assert same_bits(d.get(d_sc, np.zeros(5)), score)
        _amr.check(lib.amr_tone8_acquire_device(pl.handle, d_x, _amr.DTYPES[x.dtype], 2, n + 13, d_st, d_sh, None))   # score optional
        pl.synchronize()
        assert lib.amr_tone8_acquire_device(pl.handle, d_x, _amr.DTYPES[x.dtype], 9, n + 13, d_st, d_sh, None) == _amr.AMR_E_CAPACITY
        assert lib.amr_tone8_acquire_device(pl.handle, d_x, 7, 5, n + 13, d_st, d_sh, None) == _amr.AMR_E_INVALID
        assert lib.amr_tone8_acquire_device(pl.handle, d_x, _amr.DTYPES[x.dtype], 5, n - 1, d_st, d_sh, None) == _amr.AMR_E_INVALID
        assert lib.amr_tone8_acquire_device(pl.handle, d_x, _amr.DTYPES[x.dtype], 5, n + 13, d_st, None, None) == _amr.AMR_E_INVALID


def test_acquire_zeros_nan_and_infinities():
    L, c2, G = 80, 5, 3
    c = cfg(L, c2)
    rng = np.random.default_rng(32)
    n = 300 * 10 + 4
    x = rng.standard_normal((7, n)).astype(np.float32)
    x[0] = 0.0                                               # all zeros: every score 0, the first candidate
    x[1, 0] = np.nan                                         # in S[0][-G]: (0, -G) is kept, the score a NaN
    x[2, 1500] = np.nan                                      # elsewhere: it only removes candidates
    x[3, n - 1] = np.inf                                     # past the last slot: never read
    x[4, 17] = -np.inf
    x[5, 2000] = np.inf
    x[6] = 0.0
    x[6, 1234] = -1.5                                        # one sample alone
    start, shift, score = check_acquire(x, c, G)
    assert (start[0], shift[0], score[0]) == (0, -G, 0.0)
    assert (start[1], shift[1]) == (0, -G) and np.isnan(score[1])
    assert np.isfinite(score[2]) and np.isfinite(score[3]) and score[6] > 0


def test_peak_on_crafted_energies():
    """amr_tone8_peak_host: exact ties in j (inside a chunk and across chunks) and in g, a NaN first candidate, NaN
    elsewhere, a chunk of nothing but NaN, no start slot; random P over several chunks."""
    import _amr
    nan = np.nan
    for G in (2, 6, 16):
        C, NB, T = _amr.tone8_chunk(G), 15 + 2 * G, 10
        nw = 2 * C + 5 + 48

        def costas_at(P, j, g, v=1.0):
            for s in range(7):
                P[j + 8 * s, g + G + 2 * tc.COSTAS[s]] = v
        cases = [np.zeros((nw, NB)) for _ in range(9)]
        costas_at(cases[1], 5, 1)
        costas_at(cases[2], 5, 1); costas_at(cases[2], 9, -2)            # a tie later in j, the same chunk
        costas_at(cases[3], C + 2, 1); costas_at(cases[3], 5, -2); costas_at(cases[3], 2 * C + 1, 0)   # ties across chunks
        costas_at(cases[4], 5, 1); costas_at(cases[4], 5, -1)            # a tie in g
        costas_at(cases[5], 5, 1); cases[5][0, 2 * 3] = nan              # a NaN first candidate
        costas_at(cases[6], C + 3, 2); cases[6][20, :] = nan             # NaN elsewhere
        costas_at(cases[7], 2 * C + 2, -1); cases[7][:C + 48, :] = nan   # chunk 0 nothing but NaN: its first score too
        costas_at(cases[8], C + 1, 2, np.inf)
        P = np.stack(cases)
        start, shift, score = _amr.tone8_peak(P, T, G)
        want = [tc.peak(p, T, G) for p in P]
        assert list(start) == [w[0] for w in want] and list(shift) == [w[1] for w in want], (G, start, shift)
        assert same_bits(score, np.array([w[2] for w in want]))
        assert (start[0], shift[0]) == (0, -G) and (start[2], shift[2]) == (50, 1) and (start[3], shift[3]) == (50, -2)
        assert (start[4], shift[4]) == (50, -1) and (start[5], shift[5]) == (0, -G) and np.isnan(score[5])
        assert (start[7], shift[7]) == (0, -G) and np.isnan(score[7]) and score[8] == np.inf
        rng = np.random.default_rng(G)
        R = rng.integers(0, 3, (65, nw, NB)).astype(np.float64)         # small integers: ties everywhere
        R[rng.integers(0, 65, 40), rng.integers(0, nw, 40), rng.integers(0, NB, 40)] = nan
        start, shift, score = _amr.tone8_peak(R, T, G)
        want = [tc.peak(p, T, G) for p in R]
        assert list(start) == [w[0] for w in want] and list(shift) == [w[1] for w in want]
        assert same_bits(score, np.array([w[2] for w in want]))
        for nw0 in (0, 1, 48):                                           # no start slot
            s0, g0, v0 = _amr.tone8_peak(np.ones((2, nw0, NB)), T, G)
            assert not s0.any() and not g0.any() and not v0.any()
        s1, g1, v1 = _amr.tone8_peak(np.ones((2, 49, NB)), T, G)
        assert list(s1) == [0, 0] and list(g1) == [-G, -G] and list(v1) == [7.0, 7.0]


# ---- 2. the symbol stage alone -----------------------------------------------------------------
def want_Y(x, c, G, offs, shifts):
    with np.errstate(all="ignore"):
        return np.stack([tc.symbols(r, int(o), int(g), *c, G) for r, o, g in zip(x, offs, shifts)])


@pytest.mark.parametrize("L,c2,G", GEOS)
def test_dft_offsets_and_shifts(L, c2, G):
    """o in {0, 1, L - 1} with the last symbol cut by n, g in {-G, 0, G}, mixed per stream."""
    c = cfg(L, c2)
    rng = np.random.default_rng(7 * L + c2)
    n = 5 * L + L // 3
    x = rng.standard_normal((4, n)).astype(np.float32)
    pl = plan_for(n, c, G, 4)
    got = pl.symbols_at(x)
    assert got.shape == (4, 5, 8) and same_bits(got, want_Y(x, c, G, [0] * 4, [0] * 4))
    assert np.abs(got).max() > 0.5                           # not the zeros of a kernel that did not run
    for o in (0, 1, L - 1):
        for g in (-G, 0, G):
            offs, shifts = np.full(4, o, np.int64), np.full(4, g, np.int64)
            assert same_bits(pl.symbols_at(x, offs, shifts), want_Y(x, c, G, offs, shifts)), (o, g)
    offs, shifts = np.array([L - 1, 0, 1, L // 2], np.int64), np.array([G, -G, 0, G // 2], np.int64)
    assert same_bits(pl.symbols_at(x, offs, shifts), want_Y(x, c, G, offs, shifts))
    for bad_o, bad_g in ((-1, 0), (L, 0), (0, G + 1), (0, -G - 1)):
        with pytest.raises(Exception):
            pl.symbols_at(x, np.array([0, bad_o, 0, 0], np.int64), np.array([0, bad_g, 0, 0], np.int64))


@pytest.mark.parametrize("S", [0, 1, 63, 64, 65])
def test_dft_symbol_and_stream_counts(S):
    """Flat (symbol, tone) indices cross wave and block edges inside and between streams; n at the least that
    holds S symbols, a sample more, and a sample less than S + 1 would need."""
    L, c2, G = 24, 4, 1
    c = cfg(L, c2)
    rng = np.random.default_rng(1000 + S)
    for B, r in zip(STREAMS, (0, 1, L - 1)):
        n = S * L + r
        x = rng.standard_normal((B, n)).astype(np.float32)
        pl = plan_for(n, c, G, B)
        assert pl.S == S
        offs, shifts = rng.integers(0, L, B), rng.integers(-G, G + 1, B)
        got = pl.symbols_at(x, offs, shifts)
        assert got.shape == (B, S, 8)
        if S:
            assert same_bits(got, want_Y(x, c, G, offs, shifts)), (B, r)


@pytest.mark.parametrize("dt", ["f32", "f64", "i16"])
def test_dft_dtypes_row_stride_and_special_samples(dt):
    L, c2, G = 80, 5, 3
    c = cfg(L, c2)
    n = 8 * 80 + 45
    rng = np.random.default_rng(3)
    wide = rng.standard_normal((6, n + 13))
    if dt == "i16":
        wide = np.round(wide * 9000).astype(np.int16)
        wide[4, ::7] = ([-32768, 32767] * 60)[:len(wide[4, ::7])]
    else:
        wide[3, 100] = np.inf
        wide[3, 101] = -np.inf
        wide[4, 90] = np.nan
        wide[5] *= 1e-310 if dt == "f64" else 1e-40
        wide = wide.astype({"f32": np.float32, "f64": np.float64}[dt])
    wide[2] = 0
    x = wide[:, :n]
    pl = plan_for(n, c, G, 8)
    offs, shifts = np.array([0, 79, 6, 5, 4, 3], np.int64), np.array([0, 3, -3, 1, -1, 2], np.int64)
    assert same_bits(pl.symbols_at(x, offs, shifts), want_Y(x, c, G, offs, shifts))
    assert same_bits(pl.symbols_at(np.ascontiguousarray(x)), want_Y(x, c, G, [0] * 6, [0] * 6))


# ---- 3. the slicer and the soft stage alone ---------------------------------------------------
def want_bits(Y):
    return np.stack([tc.slice_bits(y) for y in Y])


def want_soft(Y):
    with np.errstate(all="ignore"):
        return np.stack([tc.soft(y) for y in Y])


def test_slice_and_soft_stage_sizes():
    """1 .. 100 symbols per stream: a word's 32 bits hold 10 symbols and two bits of the next."""
    import _amr
    rng = np.random.default_rng(20)
    for S in (1, 2, 10, 11, 21, 22, 43, 85, 86, 100):
        for B in (1, 3, 65):
            Y = rng.standard_normal((B, S, 8)) + 1j * rng.standard_normal((B, S, 8))
            bits, soft = _amr.tone8_slice(Y), _amr.tone8_soft(Y)
            assert bits.shape == (B, 3 * S) and np.array_equal(bits, want_bits(Y)), (S, B)
            assert soft.dtype == np.int8 and np.array_equal(soft, want_soft(Y)), (S, B)
            assert np.array_equal(soft > 0, bits.astype(bool))                       # the sign is the hard bit
    assert _amr.tone8_slice(np.ones((3, 0, 8), np.complex128)).shape == (3, 0)
    assert _amr.tone8_soft(np.ones((3, 0, 8), np.complex128)).shape == (3, 0)


def test_slice_and_soft_on_crafted_energies():
    """Exact ties between every pair of tones, all eight equal, zeros, NaN in one tone, in all, infinities, and
    components whose squares overflow or underflow."""
    import _amr
    rows = []
    for a in range(8):
        for b in range(8):
            y = np.full(8, 0.25 + 0j)
            y[a] = 1.0
            y[b] = 1j                                        # |.|^2 ties exactly with tone a
            rows.append(y)
    rows.append(np.zeros(8, np.complex128))
    rows.append(np.full(8, 3.0 - 4.0j))
    for m in range(8):
        y = np.arange(1, 9).astype(np.complex128)
        y[m] = complex(np.nan, 1.0)
        rows.append(y)
        y = np.arange(8, 0, -1).astype(np.complex128)
        y[m] = complex(0.0, np.inf)
        rows.append(y)
    rows.append(np.full(8, complex(np.nan, np.nan)))
    rows.append(np.full(8, complex(np.inf, 0.0)))
    rows.append(np.array([1e200, 1e-200, 2e200, 5e-324, 0, -0.0, 1e155, 1e154]).astype(np.complex128))
    y = np.full(8, complex(np.nan, 0.0))
    y[5] = 2.0
    rows.append(y)
    Y = np.stack(rows)[None, :, :]
    with np.errstate(all="ignore"):
        bits, soft = _amr.tone8_slice(Y), _amr.tone8_soft(Y)
        assert np.array_equal(bits, want_bits(Y)) and np.array_equal(soft, want_soft(Y))
        tones = tc.decide(Y[0])
    assert not np.any(soft == 0) and not np.any(soft == -128)
    assert tones[:64].tolist() == [min(a, b) for a in range(8) for b in range(8)]     # the first of a tie
    assert tones[64] == 0 and tones[65] == 0 and tones[-1] == 0                       # a NaN first energy keeps 0
    # the same rows as 65 streams of one symbol
    Z = np.ascontiguousarray(np.stack(rows)[:65, None, :])
    with np.errstate(all="ignore"):
        assert np.array_equal(_amr.tone8_slice(Z), want_bits(Z)) and np.array_equal(_amr.tone8_soft(Z), want_soft(Z))


# ---- 4. full demodulation -------------------------------------------------------------------
CASES = {"b12": (1200, 3000.0, 96000, 3), "l24": tc.pair_of(24, 5) + (3,)}
SIGMA = {"b12": 0.5, "l24": 0.15}
B_MAX = 67
SHORT = 5                 # streams of the float64 and int16 batches (the restatement's time)
_cases = {}


def make_batch(name, dt):
    """[B][n] streams at random delays with the sender a random number of half spacings off, under noise: frames
    whose sync word sits 0 .. 7 bits into a byte, and noise alone (no sync word)."""
    baud, carrier, fs, G = CASES[name]
    rng = np.random.default_rng(len(name) + int(baud))
    L = tc.geometry(baud, carrier, fs, G)[0]
    room = 6
    n = (7 + 3 * (room + 3) + 5) * L + 2 * L + 17
    rows = []
    for i in range(B_MAX if dt == "f32" else SHORT):
        x = np.zeros(n, np.float32)
        if i % 3 != 2:
            sh = (i // 3) % 8
            body = b"FB" + rng.integers(0, 256, room, dtype=np.uint8).tobytes()
            bits = np.concatenate([np.zeros(sh, np.uint8), np.unpackbits(np.frombuffer(body, np.uint8)),
                                   np.zeros(8 - sh, np.uint8)])
            off = int(rng.integers(-G, G + 1))
            w = tc.modulate(np.packbits(bits).tobytes(), baud, carrier + off * baud / 2, fs)
            t = int(rng.integers(0, 4 * L))
            x[t:t + w.size] = w
        rows.append(x + rng.normal(0, SIGMA[name], n))
    x = np.stack(rows)
    if dt == "i16":
        return np.round(np.clip(x, -3.9, 3.9) * 8000).astype(np.int16)
    return x.astype(np.float32 if dt == "f32" else np.float64)


def case(name, dt):
    """(x, acquired [(bytes, soft, sync, start, shift)], unacquired the same) from the restatement, once per module."""
    if (name, dt) not in _cases:
        x = make_batch(name, dt)
        baud, carrier, fs, G = CASES[name]
        _cases[name, dt] = (x, [tc.demod_soft(r, baud, carrier, fs, True, G) for r in x],
                            [tc.demod_soft(r, baud, carrier, fs, False, G) for r in x])
    return _cases[name, dt]


def test_the_cases_hold_what_they_should():
    for name in CASES:
        x, acq, plain = case(name, "f32")
        syncs = np.array([w[2] for w in acq])
        assert np.sum(syncs >= 0) >= 35 and np.sum(syncs < 0) >= 15 and all(len(w[0]) > 0 for w in acq), (name, syncs)
        assert len({int(s) % 8 for s in syncs if s >= 0}) == 8                   # every alignment of the sync word
        assert len({w[3] for w in acq}) >= 20 and len({w[4] for w in acq}) >= 5  # the delays and the shifts differ
        assert sum(a[0] != p[0] for a, p in zip(acq, plain)) > 20                # and acquisition matters


@pytest.mark.parametrize("acquire", [True, False])
@pytest.mark.parametrize("dt", ["f32", "f64", "i16"])
@pytest.mark.parametrize("name", list(CASES))
def test_demod_equals_the_restatement(name, dt, acquire):
    import _amr
    baud, carrier, fs, G = CASES[name]
    x, acq, plain = case(name, dt)
    want = acq if acquire else plain
    n = x.shape[1]
    for B in sorted({1, 3, len(x)}):
        pl = _amr.Tone8Plan(n, baud, carrier, fs, G, max_streams=B)
        assert pl.out_cap == 3 * (n // pl.L) // 8 + 1
        outs, sync, softs, starts, shifts = pl.demod_host(x[:B], soft=True, acquire=acquire)
        assert outs == [w[0] for w in want[:B]], (name, dt, B)
        assert list(sync) == [w[2] for w in want[:B]], (name, dt, B)
        assert list(starts) == [w[3] for w in want[:B]] and list(shifts) == [w[4] for w in want[:B]], (name, dt, B)
        for i, w in enumerate(want[:B]):
            assert softs[i].dtype == np.int8 and np.array_equal(softs[i], w[1]), (name, dt, B, i)
            assert np.packbits(softs[i] > 0).tobytes() == outs[i]
        hard = pl.demod_host(x[:B], acquire=acquire)
        assert hard[0] == outs and np.array_equal(hard[1], sync) and hard[2] is None
        assert np.array_equal(hard[3], starts) and np.array_equal(hard[4], shifts)
    # more streams than the plan holds: the host layer cuts the batch
    pl = _amr.Tone8Plan(n, baud, carrier, fs, G, max_streams=4)
    got = pl.demod_host(x, acquire=acquire)
    assert got[0] == [w[0] for w in want] and list(got[4]) == [w[4] for w in want]


def test_modem_functions_plan_cache_and_timings():
    import _amr
    import modem
    baud, carrier, fs, G = CASES["b12"]
    x, acq, plain = case("b12", "f32")
    n = x.shape[1]
    assert modem.tone8_demodulate_batch(x[:9], baud, carrier, search=G) == [w[0] for w in acq[:9]]
    assert modem.tone8_demodulate_batch(x[:9], baud, carrier, acquire=False) == [w[0] for w in plain[:9]]
    assert modem.tone8_demodulate(x[1], baud, carrier, search=G) == acq[1][0]
    st, sh = modem.tone8_acquire_batch(x[:9], baud, carrier, search=G)
    assert list(st) == [w[3] for w in acq[:9]] and list(sh) == [w[4] for w in acq[:9]]
    assert modem.tone8_acquire(x[4], baud, carrier, search=G) == (acq[4][3], acq[4][4])
    x16 = x[1].astype(np.float16)                            # anything but float32 / float64 / int16 goes as float64
    assert modem.tone8_demodulate(x16, baud, carrier, search=G) == tc.demod(x16, baud, carrier, fs, True, G)[0]
    so, sv = modem.tone8_demodulate_soft_batch(x[:9], baud, carrier, search=G)
    assert so == [w[0] for w in acq[:9]] and all(np.array_equal(a, w[1]) for a, w in zip(sv, acq))
    d1, s1 = modem.tone8_demodulate_soft(x[4], baud, carrier, acquire=False)
    assert d1 == plain[4][0] and np.array_equal(s1, plain[4][1])
    # a narrower search is another plan and may find another answer; the restatement says which
    assert modem.tone8_demodulate_batch(x[:5], baud, carrier, search=1) == [tc.demod(r, baud, carrier, fs, True, 1)[0] for r in x[:5]]
    # the cache counts the acquisition buffers once a plan acquires
    pl = _amr.get_tone8_plan(n, baud, carrier, G, fs, 9)
    assert pl is _amr.get_tone8_plan(n, baud, carrier, G, fs, 3) and pl.max_streams == 16
    assert pl is not _amr.get_tone8_plan(n, baud, carrier, 1, fs, 3)
    lib = _amr.lib()
    total = lib.amr_tone8_plan_bytes_estimate(n, 80, G, 16) + lib.amr_tone8_acquire_bytes_estimate(n, 80, G, 16)
    assert lib.amr_tone8_acquire_bytes_estimate(n, 80, G, 16) < pl.scratch_bytes() <= total
    fresh = _amr.Tone8Plan(n, baud, carrier, fs, G, max_streams=4)
    before = fresh.scratch_bytes()
    assert before == 2 * 80 * 16 + 4 * fresh.S * 128 + 4 * ((3 * fresh.S + 31) // 32) * 4     # E, Y, words
    fresh.demod_host(x[:4], acquire=False)
    staged = fresh.scratch_bytes()
    assert staged == lib.amr_tone8_plan_bytes_estimate(n, 80, G, 4)
    fresh.acquire(x[:4])
    assert before < staged and fresh.scratch_bytes() == staged + lib.amr_tone8_acquire_bytes_estimate(n, 80, G, 4)
    pl.enable_timing()
    pl.demod_host(x[:9], acquire=False)
    t = pl.timings()
    assert set(t) == {"despread", "slice", "sync_pack", "launch"} and all(v >= 0 for v in t.values())
    pl.demod_host(x[:9], soft=True)
    t = pl.timings()
    assert set(t) == set(_amr.TD_SLOTS) and t["launch"] >= max(t["acquire"], t["despread"], t["slice"], t["sync_pack"])
    pl.enable_timing(False)
    # the aliases stay the reference's two-tone FSK at 50 Bd
    assert np.array_equal(modem.ft8_modulate(b"FB", 1200, 1000.0), modem.fsk_modulate(b"FB", 50, 1000.0, 1050.0))


def test_no_symbol_is_empty():
    import _amr
    import modem
    rng = np.random.default_rng(1)
    baud, carrier, fs, G = CASES["b12"]
    for n in (0, 9, 79):                                     # S = 0 at L = 80
        x = rng.normal(0, 0.3, (3, n)).astype(np.float32)
        pl = _amr.Tone8Plan(n, baud, carrier, fs, G, max_streams=3)
        assert pl.out_cap == 1
        for acquire in (False, True):
            outs, sync, softs, starts, shifts = pl.demod_host(x, soft=True, acquire=acquire)
            assert outs == [b""] * 3 and list(sync) == [-1] * 3 and all(s.size == 0 for s in softs)
            assert not starts.any() and not shifts.any()
    assert modem.tone8_demodulate(np.zeros(20, np.float32), baud, carrier, search=G) == b""
    lib = _amr.lib()
    pl = _amr.Tone8Plan(100, baud, carrier, fs, G, max_streams=3)
    for acquire in (0, 1):                                   # an empty batch
        assert lib.amr_tone8_demod_host(pl.handle, None, 0, 0, 100, None, 1, None, None, None, 0, None, None, acquire) == _amr.AMR_OK
    assert lib.amr_tone8_acquire_host(pl.handle, None, 0, 0, 100, None, None, None) == _amr.AMR_OK
    assert lib.amr_tone8_symbols_at_host(pl.handle, None, 0, 0, 100, None, None, None) == _amr.AMR_OK


def test_device_entries():
    """amr_tone8_demod_device on the caller's buffers: wider rows, the soft rows pre-filled, soft, start and shift
    optional, acquired and not: the same bytes, values, starts and shifts as the host entry."""
    import _amr
    baud, carrier, fs, G = CASES["b12"]
    x, acq, plain = case("b12", "f32")
    n = x.shape[1]
    B = 65
    L = _amr.lib()
    pl = _amr.Tone8Plan(n, baud, carrier, fs, G, max_streams=B)
    cap = pl.out_cap
    xw = np.zeros((B, n + 9), np.float32)
    xw[:, :n] = x[:B]
    xw[:, n:] = np.nan                                       # the padding is never read
    F32 = _amr.DTYPE_F32
    with Dev() as d:
        d_x = d.put(xw)
        d_out, d_len, d_sync = d.put(np.zeros((B, cap + 3), np.uint8)), d.put(np.zeros(B, np.int64)), d.put(np.zeros(B, np.int64))
        d_st, d_sh = d.put(np.full(B, -5, np.int64)), d.put(np.full(B, -5, np.int64))
        for acquire, want in ((1, acq), (0, plain)):
            d_soft = d.put(np.full((B, 8 * cap + 5), 77, np.int8))
            _amr.check(L.amr_tone8_demod_device(pl.handle, d_x, F32, B, n + 9, d_out, cap + 3, d_len, d_sync, d_soft,
                                                8 * cap + 5, d_st, d_sh, acquire))
            pl.synchronize()
            out, ln, sy = d.get(d_out, np.zeros((B, cap + 3), np.uint8)), d.get(d_len, np.zeros(B, np.int64)), d.get(d_sync, np.zeros(B, np.int64))
            assert [out[i, :ln[i]].tobytes() for i in range(B)] == [w[0] for w in want[:B]]
            assert list(sy) == [w[2] for w in want[:B]]
            assert list(d.get(d_st, np.zeros(B, np.int64))) == [w[3] for w in want[:B]]
            assert list(d.get(d_sh, np.zeros(B, np.int64))) == [w[4] for w in want[:B]]
            soft = d.get(d_soft, np.zeros((B, 8 * cap + 5), np.int8))
            for i in range(B):
                assert np.array_equal(soft[i, :8 * ln[i]], want[i][1]), i
                assert np.all(soft[i, 8 * ln[i]:] == 77), i      # nothing past the stream's bytes is written
            # soft, start and shift left out
            _amr.check(L.amr_tone8_demod_device(pl.handle, d_x, F32, B, n + 9, d_out, cap + 3, d_len, d_sync, None, 0,
                                                None, None, acquire))
            pl.synchronize()
            out2, ln2 = d.get(d_out, np.zeros((B, cap + 3), np.uint8)), d.get(d_len, np.zeros(B, np.int64))
            assert np.array_equal(ln, ln2) and [out2[i, :ln[i]].tobytes() for i in range(B)] == [w[0] for w in want[:B]]
        # the argument contract, on a live plan
        args = (d_out, cap + 3, d_len, d_sync, None, 0, None, None, 1)
        assert L.amr_tone8_demod_device(pl.handle, d_x, F32, B + 1, n + 9, *args) == _amr.AMR_E_CAPACITY
        assert L.amr_tone8_demod_device(pl.handle, d_x, 7, B, n + 9, *args) == _amr.AMR_E_INVALID
        assert L.amr_tone8_demod_device(pl.handle, d_x, F32, B, n - 1, *args) == _amr.AMR_E_INVALID
        assert L.amr_tone8_demod_device(pl.handle, d_x, F32, B, n + 9, d_out, cap - 2, d_len, d_sync, None, 0, None, None, 1) == _amr.AMR_E_INVALID
        assert L.amr_tone8_demod_device(pl.handle, d_x, F32, B, n + 9, d_out, cap + 3, d_len, d_sync, d_soft, 8 * cap - 1,
                                        None, None, 1) == _amr.AMR_E_INVALID
        assert L.amr_tone8_demod_device(pl.handle, d_x, F32, 0, n + 9, *args) == _amr.AMR_OK


# ---- 5. transmit ----------------------------------------------------------------------------
TX_LENS = [0, 1, 2, 3, 5, 17, 64, 97]


@pytest.mark.parametrize("baud,carrier,fs", [(1200, 3000.0, 96000), (600, 1500.0, 96000), (50, 1000.0, 96000),
                                             tc.pair_of(24, 2), tc.pair_of(24, 9), tc.pair_of(40, 11)])
def test_modulate_batch_equals_the_restatement(baud, carrier, fs):
    """Bit-equal: the sine is the host's table.  The natural length, shorter and longer; the padding exact
    zeros; the int16 samples those of the float32 ones."""
    import modem
    rng = np.random.default_rng(int(baud) + int(carrier))
    datas = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (TX_LENS[:6] if baud == 50 else TX_LENS)]
    L = tc.geometry(baud, carrier, fs, 0)[0]
    refs = [tc.modulate(d, baud, carrier, fs) for d in datas]
    assert [r.size for r in refs] == [(7 + -(-8 * len(d) // 3)) * L for d in datas]
    natural = max(r.size for r in refs)
    for n_out in (None, natural - 2 * L - 3, natural + 37):
        want = np.zeros((len(datas), natural if n_out is None else n_out), np.float32)
        for i, r in enumerate(refs):
            k = min(r.size, want.shape[1])
            want[i, :k] = r[:k]
        got, pcm = modem.modulate_batch("tone8", datas, baud, carrier, samp_rate=fs, n_out=n_out, pcm=True)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (baud, n_out)
        assert pcm.dtype == np.int16 and np.array_equal(pcm, (want * np.float32(32767)).astype(np.int16)), (baud, n_out)
        plain = modem.modulate_batch("tone8", datas, baud, carrier, samp_rate=fs, n_out=n_out)
        assert np.array_equal(plain.view(np.uint32), want.view(np.uint32))
    one = modem.tone8_modulate(datas[5], baud, carrier, fs)
    assert np.array_equal(one.view(np.uint32), refs[5].view(np.uint32))
    assert modem.modulate_batch("tone8", [], baud, carrier, samp_rate=fs).shape == (0, 0)


# ---- 6. loopback and the coded chain --------------------------------------------------------
@pytest.mark.parametrize("baud,carrier,G", [(1200, 3000.0, 3), (600, 1500.0, 3), (2400, 12000.0, 6)])
def test_loopback_frames_parse(baud, carrier, G):
    """GPU modulator at a carrier a random number of half spacings off -> a random delay per stream -> GPU
    acquisition and demodulator tuned to `carrier` -> frame scan: every frame's payload comes back, CRC valid, the
    shifts exact and the starts within a slot of the delays; then the same under N(0, 0.1^2)."""
    import modem
    from test_gpu_loopback import _frames, _payloads, _want_payload
    seed = int(baud)
    rng = np.random.default_rng(seed)
    frames = _frames(3, 12, seed=seed)
    L = tc.geometry(baud, carrier, 96000, G)[0]
    offs = rng.integers(-G, G + 1, len(frames))
    ws = [modem.tone8_modulate(fr, baud, carrier + int(o) * baud / 2) for fr, o in zip(frames, offs)]
    delays = rng.integers(0, 5 * L, len(frames))
    x = np.zeros((len(frames), max(w.size for w in ws) + 7 * L), np.float32)
    for i, t in enumerate(delays):
        x[i, t:t + ws[i].size] = ws[i]
    for sigma in (0.0, 0.1):
        y = x + rng.normal(0, sigma, x.shape).astype(np.float32) if sigma else x
        starts, shifts = modem.tone8_acquire_batch(y, baud, carrier, search=G)
        assert list(shifts) == list(offs) and all(abs(int(s) - int(t)) <= L // 8 for s, t in zip(starts, delays))
        raws = modem.tone8_demodulate_batch(y, baud, carrier, search=G)
        assert raws == [tc.demod(r, baud, carrier, 96000, True, G)[0] for r in y]
        got = _payloads(raws)
        for i, fr in enumerate(frames):
            assert raws[i][:len(fr)] == fr and got[i] == [_want_payload(fr)], (baud, sigma, i)


def test_end_to_end_coded_chain():
    """encode_batch -> tone8 modulate, the sender off the receiver's carrier -> a random delay per stream ->
    N(0, 1.0^2) -> acquisition and soft demodulation -> decode_soft_batch returns the messages.  1200 Bd on
    3000 Hz (80 samples per symbol), search 3, 8 messages of 60 bytes, seed 8.  1.0 is the level the host
    ladder cleared at this configuration (tests/test_tone8_host.py); on the restatement every shift is exact
    there, the uncoded sync word is found in all 8 streams and all 8 messages come back.  The restatement runs
    here again, so the GPU's starts, shifts and soft values are checked at this level too."""
    import fec
    import modem
    rng = np.random.default_rng(8)
    msgs = vc.messages(rng, [60] * 8)
    cws = fec.ConvolutionalEncoder().encode_batch(msgs)
    n_cw = len(cws[0])
    assert cws == [vc.encode(m) for m in msgs]
    baud, carrier, G, L = 1200, 3000.0, 3, 80
    delays = rng.integers(0, 5 * L, 8)
    offs = rng.integers(-G, G + 1, 8)
    tx = [modem.tone8_modulate(b"FB" + c, baud, carrier + int(o) * baud / 2) for c, o in zip(cws, offs)]
    ref = [tc.modulate(b"FB" + c, baud, carrier + int(o) * baud / 2) for c, o in zip(cws, offs)]
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(tx, ref))
    x = np.zeros((8, tx[0].size + 7 * L), np.float32)
    for i, t in enumerate(delays):
        x[i, t:t + tx[i].size] = tx[i]
    x = (x.astype(np.float64) + rng.normal(0, 1.0, x.shape)).astype(np.float32)
    outs, softs = modem.tone8_demodulate_soft_batch(x, baud, carrier, search=G)
    want = [tc.demod_soft(r, baud, carrier, 96000, True, G) for r in x]
    assert [w[4] for w in want] == list(offs)
    st, sh = modem.tone8_acquire_batch(x, baud, carrier, search=G)
    assert list(st) == [w[3] for w in want] and list(sh) == list(offs)
    assert outs == [w[0] for w in want] and all(np.array_equal(s, w[1]) for s, w in zip(softs, want))
    assert all(o[:2] == b"FB" and len(o) >= 2 + n_cw for o in outs)          # sync found in all
    rows = [s[16:16 + 8 * n_cw] for s in softs]
    assert fec.ViterbiDecoder().decode_soft_batch(rows) == msgs
