"""ofdm acquisition on the GPU: k_ofdm_fold and k_ofdm_acq_min
(ofdm_acq_kernels.hip), k_ofdm_dft_at (ofdm_kernels.hip) and the plan / host
layer around them, against the numpy restatement in
tests/ofdm_acquire_cases.py.  Everything is bit-equal to the restatement."""
import ctypes

import numpy as np
import pytest

import ofdm_acquire_cases as ac
import ofdm_cases as oc
import soft_cases as sc
import viterbi_cases as vc
from test_gpu_ofdm import cfg, plan_for, same_bits, within_one_ulp_per_sine
from test_gpu_viterbi import Dev

pytestmark = pytest.mark.gpu

# (K, sps): L = 10, 15, 33, 80, 640, 1280 -- below a wave, not dividing 64, above a block of the fold
GEOS = [(1, 10), (3, 5), (3, 11), (8, 10), (64, 10), (16, 80)]
PERIODS = [0, 1, 2, 63, 64, 65, 129]
STREAMS = [1, 2, 65]


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")
    assert "amr_ofdm_acquire_host" in _amr.EXPORTS          # the restatement is only worth testing beside the product


def want_acq(x, c):
    """(offsets, dhat, E) of every row from the restatement."""
    r = [ac.acquire(row, *c) for row in x]
    return np.array([v[0] for v in r], np.int64), np.array([v[1] for v in r], np.int64), np.stack([v[2] for v in r])


def check_acquire(pl, x, c, what=None):
    off, dh, E = pl.acquire(x)
    woff, wdh, wE = want_acq(x, c)
    assert E.shape == wE.shape and same_bits(E, wE), what
    assert np.array_equal(dh, wdh) and np.array_equal(off, woff), what
    return off, dh, E


# ---- 1. the acquisition stage alone ---------------------------------------------------------
def test_the_geometries_cover_what_they_should():
    Ls = [oc.geometry(*cfg(K, sps))[1] for K, sps in GEOS]
    assert Ls == [10, 15, 33, 80, 640, 1280]
    assert [oc.geometry(*cfg(K, sps))[2] for K, sps in GEOS] == [1, 1, 4, 10, 80, 160]


@pytest.mark.parametrize("M", PERIODS)
@pytest.mark.parametrize("K,sps", GEOS)
def test_acquire_periods_tails_and_streams(K, sps, M):
    """M periods: no segment, one short, one full, one full and one short, two full and one of a single period;
    (n - Nu) % L = 0, 1, L - 1 (M = 0: n = Nu + L - 1, Nu, 1), each with 1, 2 and 65 streams; flat (stream,
    segment, r) indices cross waves and blocks at every L."""
    c = cfg(K, sps)
    sps_, L, Ncp, Nu, bins = oc.geometry(*c)
    rng = np.random.default_rng(1000 * L + M)
    for i, r in enumerate((0, 1, L - 1)):
        n = M * L + Nu + r if M else (Nu + L - 1, Nu, 1)[i]
        assert ac.periods(n, L, Nu) == M
        x = rng.standard_normal((max(STREAMS), n)).astype(np.float32)
        want = want_acq(x, c)
        for B in STREAMS:
            off, dh, E = plan_for(n, c, B).acquire(x[:B])
            assert same_bits(E, want[2][:B]), (K, sps, M, B, r)
            assert np.array_equal(dh, want[1][:B]) and np.array_equal(off, want[0][:B]), (K, sps, M, B, r)
            if M and Ncp:
                assert E.min() > 0                # not the zeros of a kernel that did not run
    # a plan larger than the batch, and a second call on it
    n = M * L + Nu + 2 if M else 5
    pl = plan_for(n, c, 70)
    x = rng.standard_normal((3, n))
    for _ in range(2):
        check_acquire(pl, x, c, (K, sps, M, "large plan"))


@pytest.mark.parametrize("dt", ["f32", "f64", "i16"])
@pytest.mark.parametrize("K,sps", [(8, 10), (3, 11), (16, 80)])
def test_acquire_dtypes_and_poisoned_padding(K, sps, dt):
    """Rows of a wider array whose padding is NaN (int16: full scale): a read past n changes E."""
    c = cfg(K, sps)
    sps_, L, Ncp, Nu, bins = oc.geometry(*c)
    n = 66 * L + Nu + 3
    rng = np.random.default_rng(L + len(dt))
    pad = 13
    wide = rng.standard_normal((5, n + pad))
    if dt == "i16":
        wide = np.round(wide * 9000).astype(np.int16)
        wide[:, n:] = 32767 * np.array([1, -1] * pad)[:pad]
    else:
        wide = wide.astype({"f32": np.float32, "f64": np.float64}[dt])
        wide[:, n:] = np.nan
    x = wide[:, :n]
    assert x.strides[0] == (n + pad) * x.itemsize
    pl = plan_for(n, c, 8)
    off, dh, E = check_acquire(pl, x, c, (K, sps, dt))
    assert not np.isnan(E).any()
    check_acquire(pl, np.ascontiguousarray(x), c, (K, sps, dt, "dense"))


def test_acquire_special_samples_and_ties():
    """+-inf, NaN, denormals; all zeros (dhat 0); one non-zero sample (the first of the tied zeros); NaN at E[0]
    and elsewhere: float64 arithmetic and the sequential rule have one answer for each."""
    c = cfg(8, 10)
    sps_, L, Ncp, Nu, bins = oc.geometry(*c)
    n = 70 * L + Nu
    rng = np.random.default_rng(4)
    x = rng.standard_normal((12, n))
    x[0] = 0.0
    x[1] = 0.0
    x[1, 3 * L + 5] = 0.5
    x[2, 95] = np.inf
    x[3, 100] = -np.inf
    x[3, 101] = np.inf
    x[4, 37] = np.nan                            # E[28 .. 37] NaN, E[0] not
    x[5, 5] = np.nan                             # E[0] NaN
    x[6] = 5e-324 * rng.integers(-3, 4, n)
    x[7] *= 1e-160                               # squares underflow to denormals and zero
    x[8] *= 1e150                                # squares near overflow
    x[9] = np.nan
    x[10, ::L] = np.nan                          # G[0] and G[L - Nu]
    x[11] = -0.0
    pl = plan_for(n, c, 12)
    with np.errstate(all="ignore"):
        off, dh, E = check_acquire(pl, x, c)
        assert dh[0] == 0 and off[0] == -(Ncp // 2) and dh[1] == 16 and dh[5] == 0 and dh[9] == 0 and dh[11] == 0
        assert np.isnan(E[4, 28:38]).all() and not np.isnan(E[4, 0]) and np.isnan(E[5, 0]) and np.isnan(E[9]).all()
        x32 = x.astype(np.float32)
        x32[6] = np.float32(1e-45) * rng.integers(-3, 4, n).astype(np.float32)
        x32[7] = (rng.standard_normal(n) * 1e-40).astype(np.float32)
        check_acquire(pl, x32, c)
    xi = np.zeros((2, n), np.int16)
    xi[1, ::7] = ([-32768, 32767] * n)[:len(xi[1, ::7])]
    check_acquire(pl, xi, c)


def test_acquire_no_prefix_and_device_entry():
    """Ncp = 0 (L = 5): E is zeros, o = 0.  amr_ofdm_acquire_device on a view into a larger NaN-filled
    allocation, dhat and E optional."""
    import _amr
    c = (19200, 24000.0, 1, 96000)
    rng = np.random.default_rng(6)
    x = rng.standard_normal((3, 203)).astype(np.float32)
    off, dh, E = check_acquire(plan_for(203, c, 3), x, c)
    assert not E.any() and not off.any() and not dh.any()
    c = cfg(8, 10)
    sps_, L, Ncp, Nu, bins = oc.geometry(*c)
    B, n, stride, lead = 65, 65 * L + Nu + 1, 65 * L + Nu + 1 + 7, 33
    x = rng.standard_normal((B, n)).astype(np.float32)
    big = np.full(lead + B * stride + 50, np.nan, np.float32)
    big[lead:lead + B * stride].reshape(B, stride)[:, :n] = x
    woff, wdh, wE = want_acq(x, c)
    pl = plan_for(n, c, B)
    lib = _amr.lib()
    with Dev() as d:
        d_big = d.put(big)
        d_x = ctypes.c_void_p(d_big.value + 4 * lead)
        d_off, d_dh, d_E = d.put(np.zeros(B, np.int64)), d.put(np.zeros(B, np.int64)), d.put(np.zeros((B, L)))
        _amr.check(lib.amr_ofdm_acquire_device(pl.handle, d_x, _amr.DTYPE_F32, B, stride, d_off, d_dh, d_E))
        pl.synchronize()
        assert np.array_equal(d.get(d_off, np.zeros(B, np.int64)), woff)
        assert np.array_equal(d.get(d_dh, np.zeros(B, np.int64)), wdh)
        assert same_bits(d.get(d_E, np.zeros((B, L))), wE)
        d_off2 = d.put(np.full(B, 99, np.int64))
        _amr.check(lib.amr_ofdm_acquire_device(pl.handle, d_x, _amr.DTYPE_F32, 3, stride, d_off2, None, None))
        pl.synchronize()
        assert d.get(d_off2, np.zeros(B, np.int64)).tolist() == woff[:3].tolist() + [99] * (B - 3)
        assert lib.amr_ofdm_acquire_device(pl.handle, d_x, _amr.DTYPE_F32, B + 1, stride, d_off, None, None) == _amr.AMR_E_CAPACITY
        assert lib.amr_ofdm_acquire_device(pl.handle, d_x, 7, B, stride, d_off, None, None) == _amr.AMR_E_INVALID
        assert lib.amr_ofdm_acquire_device(pl.handle, d_x, _amr.DTYPE_F32, B, n - 1, d_off, None, None) == _amr.AMR_E_INVALID
        assert lib.amr_ofdm_acquire_device(pl.handle, d_x, _amr.DTYPE_F32, B, stride, None, None, None) == _amr.AMR_E_INVALID
        assert lib.amr_ofdm_acquire_device(pl.handle, d_x, _amr.DTYPE_F32, 0, stride, None, None, None) == _amr.AMR_OK


def test_acquire_buffers_are_lazy_and_counted():
    import _amr
    c = cfg(8, 10)
    n = 200 * 80 + 70
    pl = plan_for(n, c, 4)
    before = pl.scratch_bytes()
    x = np.random.default_rng(8).standard_normal((4, n)).astype(np.float32)
    pl.demod_host(x)
    staged = pl.scratch_bytes()
    assert before < staged <= _amr.lib().amr_ofdm_plan_bytes_estimate(n, 10, 8, 4)
    pl.acquire(x)
    assert pl.scratch_bytes() == staged + _amr.lib().amr_ofdm_acquire_bytes_estimate(n, 10, 8, 4)
    pl.demod_host(x, acquire=True)
    assert pl.scratch_bytes() == staged + _amr.lib().amr_ofdm_acquire_bytes_estimate(n, 10, 8, 4)


# ---- 2. the DFT at offsets ------------------------------------------------------------------
def want_Y_at(x, offs, c):
    return np.stack([ac.symbols_at(r, int(o), *c) for r, o in zip(x, offs)])


@pytest.mark.parametrize("S", [1, 2, 64, 65])
@pytest.mark.parametrize("K,sps", [(8, 10), (3, 11)])
def test_dft_at_mixed_offsets(K, sps, S):
    """-Ncp, -1, 0, 1 and L - 1 - Ncp mixed in one batch; tails of 0, 1 and L - 1 samples: the last symbol of a
    stream read from a positive offset passes n by up to L - 1 - Ncp samples, which count as zeros; rows of a
    wider array with NaN behind n."""
    c = cfg(K, sps)
    sps_, L, Ncp, Nu, bins = oc.geometry(*c)
    rng = np.random.default_rng(100 * K + S)
    kinds = [-Ncp, -1, 0, 1, L - 1 - Ncp]
    for tail in (0, 1, L - 1):
        n = S * L + tail
        wide = rng.standard_normal((max(STREAMS), n + 9)).astype(np.float32)
        wide[:, n:] = np.nan
        offs = np.array([kinds[(i + S + tail) % 5] for i in range(max(STREAMS))], np.int64)
        want = want_Y_at(wide[:, :n], offs, c)
        for B in STREAMS:
            x = wide[:B, :n]
            pl = plan_for(n, c, B)
            got = pl.symbols_at(x, offs[:B])
            assert got.shape == (B, S, K) and not np.isnan(got.view(np.float64)).any(), (B, tail)
            assert same_bits(got, want[:B]), (B, tail)
            if B == 2:                           # offset 0 throughout is the plain DFT stage
                assert same_bits(pl.symbols_at(x, np.zeros(B, np.int64)), pl.symbols(x))
    # the other dtypes, every offset of the range
    n = S * L + 3
    offs = np.arange(-Ncp, L - Ncp, dtype=np.int64)
    x = rng.standard_normal((L, n))
    pl = plan_for(n, c, L)
    assert same_bits(pl.symbols_at(x, offs), want_Y_at(x, offs, c))
    xi = np.round(x * 9000).astype(np.int16)
    assert same_bits(pl.symbols_at(xi, offs), want_Y_at(xi, offs, c))


def test_dft_at_refuses_invalid_offsets():
    import _amr
    c = cfg(8, 10)
    n = 4 * 80 + 5
    pl = plan_for(n, c, 4)
    x = np.ones((4, n), np.float32)
    Y = np.full((4, 4, 8, 2), 7.0)
    lib = _amr.lib()
    for bad in (-11, 70, 1 << 40, -(1 << 40)):
        offs = np.array([0, 0, bad, 0], np.int64)
        assert lib.amr_ofdm_symbols_at_host(pl.handle, _amr.ptr(x), _amr.DTYPE_F32, 4, n, _amr.ptr(offs), _amr.ptr(Y)) == _amr.AMR_E_INVALID
        assert b"offset" in lib.amr_last_error() and (Y == 7.0).all()
    for ok in (-10, 69):
        offs = np.array([0, 0, ok, 0], np.int64)
        _amr.check(lib.amr_ofdm_symbols_at_host(pl.handle, _amr.ptr(x), _amr.DTYPE_F32, 4, n, _amr.ptr(offs), _amr.ptr(Y)))
    assert lib.amr_ofdm_symbols_at_host(pl.handle, _amr.ptr(x), _amr.DTYPE_F32, 4, n, None, _amr.ptr(Y)) == _amr.AMR_E_INVALID
    assert lib.amr_ofdm_symbols_at_host(pl.handle, _amr.ptr(x), _amr.DTYPE_F32, 5, n, _amr.ptr(offs), _amr.ptr(Y)) == _amr.AMR_E_CAPACITY


# ---- 3. acquire=True demodulation -----------------------------------------------------------
CASES = [(baud, carrier, K, sigma) for baud, carrier in oc.CONFIGS for K in (1, 3, 4, 8) for sigma in (0.0, 0.05)]
_cases = {}


def host_case(baud, carrier, K, sigma):
    """The host test's capture of this configuration (same seed, same draws), and its payload and delay."""
    rng = np.random.default_rng(7 + int(baud) + 100 * K + int(sigma * 100))
    L = oc.geometry(baud, carrier, K)[1]
    msg = b"FBPC" + rng.integers(0, 256, int(rng.integers(20, 201)), dtype=np.uint8).tobytes()
    t = int(rng.integers(0, 5 * L))
    return ac.delayed(msg, t, baud, carrier, K, sigma=sigma, rng=rng), msg, t


def case(i, dt):
    """(x, msg, t, (bytes, soft, sync, o) from the restatement chain), computed once per module."""
    if (i, dt) not in _cases:
        baud, carrier, K, sigma = CASES[i]
        x, msg, t = host_case(*CASES[i])
        if dt == "i16":
            x = np.round(np.clip(x, -3.9, 3.9) * 8000).astype(np.int16)
        _cases[i, dt] = (x, msg, t, ac.demod_soft(x, baud, carrier, K))
    return _cases[i, dt]


@pytest.mark.parametrize("dt", ["f32", "i16"])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_demod_acquire_equals_the_restatement(i, dt):
    import _amr
    baud, carrier, K, sigma = CASES[i]
    x, msg, t, (data, soft, sync, o) = case(i, dt)
    if oc.geometry(baud, carrier, K)[2]:
        assert sync >= 0 and data[:len(msg)] == msg          # the host test's claim, on this dtype too
    else:                                                    # L = 5 has no prefix: nothing to acquire
        assert o == 0 and (data, sync) == oc.demod(x, baud, carrier, K)
    pl = _amr.OfdmPlan(x.size, baud, carrier, K, max_streams=2)
    xb = np.stack([x, x[::-1]])                              # and a stream that is no frame at all
    w1 = ac.demod_soft(xb[1], baud, carrier, K)
    outs, syncs, offs = pl.demod_host(xb, acquire=True)
    assert outs == [data, w1[0]] and list(syncs) == [sync, w1[2]] and list(offs) == [o, w1[3]]
    souts, ssyncs, softs, soffs = pl.demod_soft_host(xb, acquire=True)
    assert souts == outs and np.array_equal(ssyncs, syncs) and np.array_equal(soffs, offs)
    assert np.array_equal(softs[0], soft) and np.array_equal(softs[1], w1[1])
    # acquire=False on the same plan afterwards is today's demodulation
    outs0, syncs0 = pl.demod_host(xb)
    assert (outs0[0], syncs0[0]) == oc.demod(x, baud, carrier, K)


def test_demod_acquire_device_entry_and_timings():
    """amr_ofdm_demod_acq_device on a view into a larger NaN-filled allocation: bytes, lengths, sync indices,
    soft values and offsets as the restatement's; soft and offset optional; the acquire timing slot."""
    import _amr
    baud, carrier, K = 9600, 12000.0, 8
    L = oc.geometry(baud, carrier, K)[1]
    rng = np.random.default_rng(31)
    B, lead, pad = 65, 17, 9
    msgs = [b"FBPC" + rng.integers(0, 256, 60, dtype=np.uint8).tobytes() for _ in range(B)]
    ts = rng.integers(0, 5 * L, B)
    n = 5 * L + oc.n_symbols(64, K) * L + L
    x = np.zeros((B, n), np.float32)
    for i in range(B):
        w = oc.modulate(msgs[i], baud, carrier, K)
        x[i, ts[i]:ts[i] + w.size] = w
    x += rng.normal(0, 0.05, x.shape).astype(np.float32)
    want = [ac.demod_soft(r, baud, carrier, K) for r in x]
    assert all(w[2] >= 0 and w[0][:64] == m for w, m in zip(want, msgs))
    stride = n + pad
    big = np.full(lead + B * stride + 40, np.nan, np.float32)
    big[lead:lead + B * stride].reshape(B, stride)[:, :n] = x
    pl = _amr.OfdmPlan(n, baud, carrier, K, max_streams=B)
    cap = pl.out_cap
    lib = _amr.lib()
    with Dev() as d:
        d_big = d.put(big)
        d_x = ctypes.c_void_p(d_big.value + 4 * lead)
        d_out, d_len, d_sync = d.put(np.zeros((B, cap + 3), np.uint8)), d.put(np.zeros(B, np.int64)), d.put(np.zeros(B, np.int64))
        d_soft, d_off = d.put(np.full((B, 8 * cap + 5), 77, np.int8)), d.put(np.zeros(B, np.int64))
        pl.enable_timing()
        _amr.check(lib.amr_ofdm_demod_acq_device(pl.handle, d_x, _amr.DTYPE_F32, B, stride, d_out, cap + 3, d_len, d_sync,
                                                 d_soft, 8 * cap + 5, d_off))
        pl.synchronize()
        tm = pl.timings()
        assert set(tm) == {"dft", "slice", "sync_pack", "launch", "acquire"} and all(v >= 0 for v in tm.values())
        assert tm["launch"] >= max(tm["dft"], tm["acquire"])
        pl.enable_timing(False)
        out, ln, sy = d.get(d_out, np.zeros((B, cap + 3), np.uint8)), d.get(d_len, np.zeros(B, np.int64)), d.get(d_sync, np.zeros(B, np.int64))
        soft, off = d.get(d_soft, np.zeros((B, 8 * cap + 5), np.int8)), d.get(d_off, np.zeros(B, np.int64))
        for i, (data, sv, sync, o) in enumerate(want):
            assert out[i, :ln[i]].tobytes() == data and sy[i] == sync and off[i] == o, i
            assert np.array_equal(soft[i, :8 * ln[i]], sv) and np.all(soft[i, 8 * ln[i]:] == 77), i
        # soft and offset are optional
        d_out2, d_len2 = d.put(np.zeros((B, cap), np.uint8)), d.put(np.zeros(B, np.int64))
        _amr.check(lib.amr_ofdm_demod_acq_device(pl.handle, d_x, _amr.DTYPE_F32, B, stride, d_out2, cap, d_len2, d_sync,
                                                 None, 0, None))
        pl.synchronize()
        out2, ln2 = d.get(d_out2, np.zeros((B, cap), np.uint8)), d.get(d_len2, np.zeros(B, np.int64))
        assert np.array_equal(ln2, ln) and all(out2[i, :ln[i]].tobytes() == want[i][0] for i in range(B))
        # the unacquired entry on the same plan is unchanged by all this
        _amr.check(lib.amr_ofdm_demod_device(pl.handle, d_x, _amr.DTYPE_F32, B, stride, d_out2, cap, d_len2, d_sync))
        pl.synchronize()
        out2, ln2 = d.get(d_out2, np.zeros((B, cap), np.uint8)), d.get(d_len2, np.zeros(B, np.int64))
        assert all(out2[i, :ln2[i]].tobytes() == oc.demod(x[i], baud, carrier, K)[0] for i in range(0, B, 8))
        # the argument contract is amr_ofdm_demod_soft_device's
        args = (d_out, cap + 3, d_len, d_sync, d_soft)
        acq = lib.amr_ofdm_demod_acq_device
        assert acq(pl.handle, d_x, _amr.DTYPE_F32, B + 1, stride, *args, 8 * cap + 5, d_off) == _amr.AMR_E_CAPACITY
        assert acq(pl.handle, d_x, 7, B, stride, *args, 8 * cap + 5, d_off) == _amr.AMR_E_INVALID
        assert acq(pl.handle, d_x, _amr.DTYPE_F32, B, n - 1, *args, 8 * cap + 5, d_off) == _amr.AMR_E_INVALID
        assert acq(pl.handle, d_x, _amr.DTYPE_F32, B, stride, d_out, cap - 2, d_len, d_sync, d_soft, 8 * cap + 5, d_off) == _amr.AMR_E_INVALID
        assert acq(pl.handle, d_x, _amr.DTYPE_F32, B, stride, *args, 8 * cap - 1, d_off) == _amr.AMR_E_INVALID
        assert acq(pl.handle, d_x, _amr.DTYPE_F32, B, stride, None, cap + 3, d_len, d_sync, None, 0, None) == _amr.AMR_E_INVALID
        assert acq(pl.handle, d_x, _amr.DTYPE_F32, 0, stride, *args, 8 * cap + 5, d_off) == _amr.AMR_OK


def test_a_delayed_capture_needs_acquisition():
    """What the feature is for: a capture that starts 30 samples into a symbol of L = 80 does not contain its
    payload without acquisition, and does with it; an aligned capture gives today's bytes either way."""
    import _amr
    import modem
    baud, carrier, K = 9600, 12000.0, 8
    sps, L, Ncp, Nu, bins = oc.geometry(baud, carrier, K)
    rng = np.random.default_rng(30)
    msg = b"FBPC" + rng.integers(0, 256, 120, dtype=np.uint8).tobytes()
    w = oc.modulate(msg, baud, carrier, K)
    late = np.concatenate([np.zeros(2 * L, np.float32), w, np.zeros(L, np.float32)])[30:]     # starts 30 samples into a symbol
    assert (L, Ncp) == (80, 10)
    plain = modem.ofdm_demodulate(late, baud, carrier, K)
    assert plain == oc.demod(late, baud, carrier, K)[0] and msg not in plain
    got = modem.ofdm_demodulate(late, baud, carrier, K, acquire=True)
    assert got == ac.demod(late, baud, carrier, K)[0] and got[:len(msg)] == msg
    assert modem.ofdm_acquire(late, baud, carrier, K) == ac.acquire(late, baud, carrier, K)[0] == 50 - Ncp // 2
    aligned = np.concatenate([w, np.zeros(L, np.float32)])
    assert modem.ofdm_acquire(aligned, baud, carrier, K) == -(Ncp // 2)
    assert modem.ofdm_demodulate(aligned, baud, carrier, K, acquire=True) == modem.ofdm_demodulate(aligned, baud, carrier, K)
    # the batched and soft forms, and the plan cache's reservation
    xb = np.stack([late, np.roll(late, 7)])
    want = [ac.demod_soft(r, baud, carrier, K) for r in xb]
    assert modem.ofdm_acquire_batch(xb, baud, carrier, K).tolist() == [w_[3] for w_ in want]
    assert modem.ofdm_demodulate_batch(xb, baud, carrier, K, acquire=True) == [w_[0] for w_ in want]
    outs, softs = modem.ofdm_demodulate_soft_batch(xb, baud, carrier, K, acquire=True)
    assert outs == [w_[0] for w_ in want] and all(np.array_equal(s, w_[1]) for s, w_ in zip(softs, want))
    d1, s1 = modem.ofdm_demodulate_soft(late, baud, carrier, K, acquire=True)
    assert d1 == want[0][0] and np.array_equal(s1, want[0][1])
    pl = _amr.get_ofdm_plan(late.size, baud, carrier, K, 96000, 2)
    assert pl.acquires and pl.scratch_bytes() <= (_amr.lib().amr_ofdm_plan_bytes_estimate(late.size, 10, K, 2) +
                                                  _amr.lib().amr_ofdm_acquire_bytes_estimate(late.size, 10, K, 2))


def test_end_to_end_coded_chain_at_random_delays():
    """test_gpu_ofdm.test_end_to_end_coded_chain's chain (16 messages of 120 bytes, 9600 Bd, 12 kHz, K = 8,
    seed 8) with every message delayed by its own random t < 5 L inside a capture 6 L longer than the frame,
    noise on all of it: acquisition, soft demodulation and the soft decoder return all 16.

    The noise is N(0, 0.13^2), not that test's 0.14.  The level was picked as that test picked its own, by
    running this chain's restatement on the CPU (ofdm_cases.modulate -> ofdm_acquire_cases.demod_soft ->
    soft_cases.soft_decode_batch) at 0.10 .. 0.14 with seeds 7, 8, 9.  The timing was exact in all 240 streams;
    what sets the limit is again the uncoded 16-bit sync word, and the window that starts half a prefix early
    sees other noise samples than the aligned chain's: at 0.14 one stream of seed 8 and one of seed 9 lose it
    (a single flipped bit inside the word), seed 9 loses one from 0.11 on, seed 7 none.  At 0.13 and seed 8
    the sync word is found in all 16 streams, every one of the 16 hard codewords has byte errors and the soft
    decoder returns all 16 messages.  The restatement runs here again, so the GPU's values are checked at
    this level too."""
    import fec
    import modem
    baud, carrier, K = 9600, 12000.0, 8
    Lsym = oc.geometry(baud, carrier, K)[1]
    rng = np.random.default_rng(8)
    msgs = vc.messages(rng, [120] * 16)
    cws = fec.ConvolutionalEncoder().encode_batch(msgs)
    Lc = len(cws[0])
    tx = modem.modulate_batch("ofdm", [b"FB" + c for c in cws], baud=baud, f0=carrier, num_subcarriers=K)
    ref = np.stack([oc.modulate(b"FB" + c, baud, carrier, K) for c in cws])
    within_one_ulp_per_sine(tx, ref, "coded chain")          # the level was picked on the restatement's samples
    ts = rng.integers(0, 5 * Lsym, 16)
    x = np.zeros((16, tx.shape[1] + 6 * Lsym))
    for i in range(16):
        x[i, ts[i]:ts[i] + tx.shape[1]] = tx[i]
    x = (x + rng.normal(0, 0.13, x.shape)).astype(np.float32)
    outs, softs = modem.ofdm_demodulate_soft_batch(x, baud, carrier, K, acquire=True)
    want = [ac.demod_soft(r, baud, carrier, K) for r in x]
    assert outs == [w[0] for w in want] and all(np.array_equal(s, w[1]) for s, w in zip(softs, want))
    assert [(w[3] + 5 - int(t)) % Lsym for w, t in zip(want, ts)] == [0] * 16        # the timing is exact
    assert all(o[:2] == b"FB" and len(o) >= 2 + Lc for o in outs)          # sync found in all
    assert all(o[2:2 + Lc] != c for o, c in zip(outs, cws))                # and every hard codeword is damaged
    rows = [s[16:16 + 8 * Lc] for s in softs]
    assert [m for m, _ in sc.soft_decode_batch(rows)] == msgs
    assert fec.ViterbiDecoder().decode_soft_batch(rows) == msgs


# ---- 4. the host layer ofdm shares with spread (sym_plan.h), at a small shape ----------------
# K = 3, sps = 4: L = 12, Ncp = 1; five symbols and a tail of 3: 24 bits, out_cap 4.  The same cases as
# test_gpu_spread.py's section 7.
SMALL = cfg(3, 4)
SMALL_N = 5 * 12 + 3
_small = {}


def small(dt):
    """(five rows of a wider array, poisoned behind n; the restatement's acquired (bytes, soft, sync, o) and
    unacquired (bytes, soft, sync) of every row), computed once per module."""
    if dt not in _small:
        wide = np.random.default_rng(12).normal(0, 0.3, (5, SMALL_N + 4))
        wide = np.round(wide * 8000).astype(np.int16) if dt == "i16" else wide.astype(np.float32)
        wide[:, SMALL_N:] = 32767 if dt == "i16" else np.nan
        x = wide[:, :SMALL_N]
        _small[dt] = (x, [ac.demod_soft(r, *SMALL) for r in x], [oc.demod_soft(r, *SMALL) for r in x])
    return _small[dt]


@pytest.mark.parametrize("dt", ["f32", "i16"])
def test_small_two_batches_of_wider_rows(dt):
    """Five streams through a plan of three (a full batch and a short one), x_stride > n: every host entry."""
    from test_gpu_ofdm import want_Y
    x, acq, plain = small(dt)
    assert oc.geometry(*SMALL)[1:3] == (12, 1) and x.strides[0] == (SMALL_N + 4) * x.itemsize
    assert all(len(w[0]) == 3 for w in plain)
    pl = plan_for(SMALL_N, SMALL, 3)
    assert pl.out_cap == 4
    outs, syncs = pl.demod_host(x)
    assert outs == [w[0] for w in plain] and list(syncs) == [w[2] for w in plain]
    outs, syncs, softs = pl.demod_soft_host(x)
    assert outs == [w[0] for w in plain] and list(syncs) == [w[2] for w in plain]
    assert all(s.dtype == np.int8 and np.array_equal(s, w[1]) for s, w in zip(softs, plain))
    outs, syncs, softs, offs = pl.demod_acq_host(x, soft=True)
    assert outs == [w[0] for w in acq] and list(syncs) == [w[2] for w in acq] and list(offs) == [w[3] for w in acq]
    assert all(np.array_equal(s, w[1]) for s, w in zip(softs, acq))
    outs, syncs, offs = pl.demod_host(x, acquire=True)
    assert outs == [w[0] for w in acq] and list(syncs) == [w[2] for w in acq] and list(offs) == [w[3] for w in acq]
    off, dh, E = check_acquire(pl, x, SMALL, dt)
    assert list(off) == [w[3] for w in acq]
    assert same_bits(pl.symbols(x), want_Y(x, SMALL))
    assert same_bits(pl.symbols_at(x, off), want_Y_at(x, off, SMALL))


@pytest.mark.parametrize("dt", ["f32", "i16"])
def test_small_host_soft_rows_are_cut(dt):
    """soft_stride above 8 * out_cap with a sentinel in the slack, out_stride at its minimum: the row is cut at
    8 * out_len[i] and nothing behind it is written."""
    import _amr
    x, acq, plain = small(dt)
    x = np.ascontiguousarray(x[:3])
    pl = plan_for(SMALL_N, SMALL, 3)
    lib, cap = _amr.lib(), pl.out_cap
    for acquire, want in ((False, plain), (True, acq)):
        out, ln, sy = np.zeros((3, cap - 1), np.uint8), np.zeros(3, np.int64), np.zeros(3, np.int64)
        soft, off = np.full((3, 8 * cap + 5), 77, np.int8), np.full(3, -99, np.int64)
        args = (pl.handle, _amr.ptr(x), _amr.DTYPES[x.dtype], 3, SMALL_N, _amr.ptr(out), cap - 1, _amr.ptr(ln),
                _amr.ptr(sy), _amr.ptr(soft), 8 * cap + 5)
        _amr.check(lib.amr_ofdm_demod_acq_host(*args, _amr.ptr(off)) if acquire else lib.amr_ofdm_demod_soft_host(*args))
        assert [out[i, :ln[i]].tobytes() for i in range(3)] == [w[0] for w in want[:3]]
        assert list(sy) == [w[2] for w in want[:3]] and list(ln) == [len(w[0]) for w in want[:3]] and min(ln) > 0
        if acquire:
            assert list(off) == [w[3] for w in want[:3]]
        for i in range(3):
            assert np.array_equal(soft[i, :8 * ln[i]], want[i][1]) and np.all(soft[i, 8 * ln[i]:] == 77), (acquire, i)


def test_small_empty_batch_and_fewer_than_two_symbols():
    import _amr
    lib = _amr.lib()
    pl = plan_for(SMALL_N, SMALL, 3)
    h, F32 = pl.handle, _amr.DTYPE_F32
    assert lib.amr_ofdm_demod_host(h, None, F32, 0, SMALL_N, None, 4, None, None) == _amr.AMR_OK
    assert lib.amr_ofdm_demod_soft_host(h, None, F32, 0, SMALL_N, None, 4, None, None, None, 32) == _amr.AMR_OK
    assert lib.amr_ofdm_demod_acq_host(h, None, F32, 0, SMALL_N, None, 4, None, None, None, 0, None) == _amr.AMR_OK
    assert lib.amr_ofdm_acquire_host(h, None, F32, 0, SMALL_N, None, None, None) == _amr.AMR_OK
    assert lib.amr_ofdm_symbols_at_host(h, None, F32, 0, SMALL_N, None, None) == _amr.AMR_OK
    rng = np.random.default_rng(3)
    for n in (3, 12 + 3):                                    # S = 0, 1
        x = rng.normal(0, 0.3, (5, n)).astype(np.float32)
        pl = plan_for(n, SMALL, 3)
        assert pl.out_cap == 1
        assert pl.demod_host(x)[0] == [b""] * 5 and list(pl.demod_host(x)[1]) == [-1] * 5
        outs, syncs, softs, offs = pl.demod_acq_host(x, soft=True)
        assert outs == [b""] * 5 and list(syncs) == [-1] * 5 and all(s.size == 0 for s in softs)
        assert list(offs) == [ac.acquire(r, *SMALL)[0] for r in x]


def test_small_scratch_bytes_are_the_estimates():
    import _amr
    x = small("f32")[0]
    lib = _amr.lib()
    plan_b, acq_b = lib.amr_ofdm_plan_bytes_estimate(SMALL_N, 4, 3, 3), lib.amr_ofdm_acquire_bytes_estimate(SMALL_N, 4, 3, 3)
    pl = plan_for(SMALL_N, SMALL, 3)
    # W [Nu][K][2], Y [ms][S][K][2], words [ms][1]: the plan before any call
    assert pl.scratch_bytes() == 11 * 3 * 16 + 3 * 5 * 3 * 16 + 3 * 4
    pl.demod_host(x)
    assert pl.scratch_bytes() == plan_b                      # + x [ms][n] doubles, out [ms][cap], len and sync [ms]
    assert plan_b == 11 * 3 * 16 + 3 * 5 * 3 * 16 + 3 * 4 + 3 * SMALL_N * 8 + 3 * 4 + 2 * 3 * 8
    pl.demod_host(x, acquire=True)
    assert pl.scratch_bytes() == plan_b + acq_b              # + gq [ms][1][L], G and E [ms][L], dhat and off [ms]
    assert acq_b == 3 * 12 * 8 + 2 * 3 * 12 * 8 + 2 * 3 * 8
    pl.acquire(x)
    pl.demod_soft_host(x)
    assert pl.scratch_bytes() == plan_b + acq_b


def test_small_plans_come_and_go():
    """Create, demodulate twice on the host (the staging allocated, then reused), destroy; a few times over."""
    x, acq, plain = small("f32")
    for k in range(3):
        pl = plan_for(SMALL_N, SMALL, 3)
        for _ in range(2):
            assert pl.demod_host(x)[0] == [w[0] for w in plain]
            assert pl.demod_host(x, acquire=True)[0] == [w[0] for w in acq]
        del pl
