"""d8psk on the GPU: k_slice8 and k_psk_soft8 (psk8_kernels.hip),
the AMR_TX_D8PSK kernels (tx_kernels.hip) and the plan / host layer around
them against the numpy restatement in tests/psk8_cases.py.  The receive side
is bit-equal to the restatement; the transmit samples are under
test_gpu_tx.assert_close's rule (sin's last ulp)."""
import numpy as np
import pytest

import psk8_cases as p8
import soft_cases as sc
import viterbi_cases as vc
from test_gpu_tx import assert_close
from test_gpu_viterbi import Dev

pytestmark = pytest.mark.gpu

B_MAX = 130
LENGTHS = {2110: (19200, 24000.0), 4097: (9600, 12000.0), 9613: (2400, 3000.0)}     # n -> (baud, carrier)
DTYPES = ["f32", "f64", "pcm16", "raw16"]
# products per stream: 10 / 11 and 21 / 22 are the tribits that straddle words, 32 / 33 k_slice8's unit edge
PRODUCTS = [1, 2, 10, 11, 21, 22, 31, 32, 33, 64, 65, 131]
STREAMS = [1, 3, 64, 65, 67]


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")
    assert _amr.PSK_KINDS["d8psk"] == _amr.PSK_D8PSK         # the restatement is only worth testing beside the product


def want_bits(sym):
    return np.stack([p8.slice_bits(r) for r in np.atleast_2d(sym)])


def want_soft(sym):
    return np.stack([p8.soft(r) for r in np.atleast_2d(sym)])


# ---- 1. the slicer and the soft stage alone -----------------------------------------
def test_slicer_stage_sizes():
    import _amr
    rng = np.random.default_rng(80)
    for nd in PRODUCTS:
        for B in STREAMS:
            sym = rng.standard_normal((B, nd + 1)) + 1j * rng.standard_normal((B, nd + 1))
            got = _amr.psk_slice("d8psk", sym)
            assert got.shape == (B, 3 * nd) and np.array_equal(got, want_bits(sym)), (nd, B)
    assert _amr.psk_slice("d8psk", np.ones((3, 1), np.complex128)).shape == (3, 0)       # S = 1: nothing
    assert _amr.psk_soft("d8psk", np.ones((3, 1), np.complex128)).shape == (3, 0)


def test_soft_stage_sizes():
    import _amr
    rng = np.random.default_rng(81)
    for nd in PRODUCTS:
        for B in (1, 65):
            sym = rng.standard_normal((B, nd + 1)) + 1j * rng.standard_normal((B, nd + 1))
            got = _amr.psk_soft("d8psk", sym)
            assert got.dtype == np.int8 and got.shape == (B, 3 * nd), (nd, B)
            assert np.array_equal(got, want_soft(sym)), (nd, B)
            assert np.array_equal(got > 0, _amr.psk_slice("d8psk", sym).astype(bool))     # the sign is the hard bit


def boundary_products():
    """ai == T * ar exactly and one ulp to each side, ar == T * ai likewise, in every quadrant: the eight
    boundary directions; then zeros, denormals, 2^+-1000, infinities and NaN in either component."""
    rng = np.random.default_rng(82)
    a = np.concatenate([10.0 ** rng.uniform(-3, 3, 40), [1.0, 0.75, 3.0, 2.0 ** -1000, 2.0 ** 900]])
    t = p8.T * a
    d = []
    for other in (t, np.nextafter(t, 0.0), np.nextafter(t, np.inf)):
        for sa in (1.0, -1.0):
            for so in (1.0, -1.0):
                d.append(sa * a + 1j * so * other)           # around pi/8, 7pi/8, -pi/8, -7pi/8
                d.append(so * other + 1j * sa * a)           # around 3pi/8, 5pi/8, -3pi/8, -5pi/8
    v = [0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1040, 2.0 ** -1000, -2.0 ** -1000, 2.0 ** 1000, -2.0 ** 1000, np.inf,
         -np.inf, np.nan, 1.0, -1.0]
    d.append(np.array([complex(x, y) for x in v for y in v]))
    return np.concatenate(d)


def test_boundary_and_special_products():
    import _amr
    d = boundary_products()
    sym = np.empty(2 * d.size + 1, np.complex128)
    sym[0::2] = 1.0
    sym[1::2] = d
    # the product of (1, d) is d itself wherever d is finite: the cases decide what they are meant to
    prod = sc.diff_products(sym)[0::2]
    fin = np.isfinite(d.real) & np.isfinite(d.imag)
    assert np.array_equal(prod[fin], d[fin]) and fin.sum() > 600
    m = p8.steps(prod)
    n = 45
    assert set(m[:8 * n].tolist()) == {1, 3, 5, 7}           # an exact tie falls to the diagonal sectors
    assert set(m[8 * n:16 * n].tolist()) == {0, 2, 4, 6}     # an ulp towards the axis
    assert set(m[16 * n:24 * n].tolist()) == {1, 3, 5, 7}
    for B in (1, 2):
        s2 = np.stack([sym] * B)
        bits, soft = _amr.psk_slice("d8psk", s2), _amr.psk_soft("d8psk", s2)
        for i in range(B):
            assert np.array_equal(bits[i], p8.slice_bits(sym)), i
            assert np.array_equal(soft[i], p8.soft(sym)), i
    assert not np.any(soft == 0) and not np.any(soft == -128)
    assert np.abs(soft[0].astype(np.int64))[2::3].max() <= 75                          # b0 tops out near 74


# ---- 2. full demodulation ---------------------------------------------------------------
def make_batch(n, dt):
    """[B_MAX][n] streams: payloads whose sync word sits 0, 1 and 2 bits into a tribit, and noise alone."""
    baud, carrier = LENGTHS[n]
    rng = np.random.default_rng(n)
    sps = 96000 // baud
    room = 3 * (n // sps - 41) // 8 - 4
    assert room >= 4
    rows = []
    for i in range(B_MAX):
        body = b"FB" + rng.integers(0, 256, room, dtype=np.uint8).tobytes()
        if i % 3 == 2:
            x = np.zeros(n, np.float32)
        else:
            shift = (i // 3) % 3
            bits = np.concatenate([np.zeros(shift, np.uint8), np.unpackbits(np.frombuffer(body, np.uint8)),
                                   np.zeros(8 - shift, np.uint8)])
            w = p8.modulate(np.packbits(bits).tobytes(), baud, carrier)
            x = np.concatenate([w, np.zeros(max(0, n - w.size), np.float32)])[:n]
        rows.append(x + rng.normal(0, 0.1, n))
    x = np.stack(rows)
    if dt in ("pcm16", "raw16"):
        return np.round(np.clip(x, -3.9, 3.9) * 8000).astype(np.int16)
    return x.astype(np.float32 if dt == "f32" else np.float64)


_cases = {}


def case(n, dt):
    """(x, [(bytes, soft, sync)] from the restatement), computed once per module."""
    if (n, dt) not in _cases:
        baud, carrier = LENGTHS[n]
        x = make_batch(n, dt)
        want = [p8.demod_soft(x[i], baud, carrier, raw_int16=dt == "raw16") for i in range(B_MAX)]
        _cases[n, dt] = (x, want)
    return _cases[n, dt]


def run(pl, x, dt, soft=False):
    if dt == "raw16":
        return pl.demod_soft_host_raw(x) if soft else pl.demod_host_raw(x)
    return pl.demod_soft_host(x) if soft else pl.demod_host(x)


def test_the_cases_hold_what_they_should():
    for n in LENGTHS:
        _, want = case(n, "f32")
        syncs = np.array([w[2] for w in want])
        assert all(np.sum((syncs >= 0) & (syncs % 3 == r)) >= 20 for r in range(3)), (n, syncs)
        assert np.sum(syncs < 0) >= 30 and all(len(w[0]) > 0 for w in want), n
        assert all(p8.demod(x, *LENGTHS[n])[0] == w[0] for x, w in zip(case(n, "f32")[0][:4], want))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", list(LENGTHS))
def test_demod_equals_the_restatement(n, dt):
    import _amr
    baud, carrier = LENGTHS[n]
    x, want = case(n, dt)
    for layout, B in (("row", 3), ("lane", 65), ("lane", B_MAX), ("split", 3)):
        pl = _amr.PskPlan("d8psk", n, baud, carrier, max_streams=B)
        pl.set_layout(layout)
        outs, sync = run(pl, x[:B], dt)
        assert pl.last_layout() == ("row" if layout == "split" else layout), (n, dt, layout)
        if layout == "lane":
            assert pl.last_lowpass() == "lane"               # never the fused slicers: they decide QPSK / BPSK
        assert outs == [w[0] for w in want[:B]], (n, dt, layout, B)
        assert list(sync) == [w[2] for w in want[:B]], (n, dt, layout, B)


@pytest.mark.parametrize("dt", ["f32", "raw16"])
@pytest.mark.parametrize("n", list(LENGTHS))
def test_demod_soft_equals_the_restatement(n, dt):
    import _amr
    baud, carrier = LENGTHS[n]
    x, want = case(n, dt)
    for layout, B in (("row", 3), ("lane", 67), ("split", 2)):
        pl = _amr.PskPlan("d8psk", n, baud, carrier, max_streams=B)
        pl.set_layout(layout)
        hard = run(pl, x[:B], dt)
        outs, sync, softs = run(pl, x[:B], dt, soft=True)
        assert outs == hard[0] and np.array_equal(sync, hard[1])
        for i, (data, soft, sy) in enumerate(want[:B]):
            assert outs[i] == data and sync[i] == sy, (n, dt, layout, i)
            assert softs[i].dtype == np.int8 and np.array_equal(softs[i], soft), (n, dt, layout, i)
            assert np.packbits(softs[i] > 0).tobytes() == outs[i], (n, dt, layout, i)


def test_modem_functions_and_the_default_layout():
    import modem
    n = 4097
    baud, carrier = LENGTHS[n]
    x, want = case(n, "f32")
    outs = modem.d8psk_demodulate_batch(x[:9], baud, carrier)
    assert outs == [w[0] for w in want[:9]]
    assert modem.d8psk_demodulate(x[1], baud, carrier) == want[1][0]
    so, sv = modem.d8psk_demodulate_soft_batch(x[:9], baud, carrier)
    assert so == outs and all(np.array_equal(a, w[1]) for a, w in zip(sv, want))
    d1, s1 = modem.d8psk_demodulate_soft(x[4], baud, carrier)
    assert d1 == want[4][0] and np.array_equal(s1, want[4][1])
    ragged = [x[0], x[1].astype(np.float64), case(2110, "f32")[0][0]]
    assert modem.demodulate_ragged("d8psk", ragged[:2], baud, carrier) == [want[0][0], want[1][0]]
    assert modem.demodulate_ragged("d8psk", ragged[2:], *LENGTHS[2110]) == [case(2110, "f32")[1][0][0]]
    # the aliases stay the reference's QPSK
    assert modem.psk8_demodulate(x[0], baud, carrier) == modem.qpsk_demodulate(x[0], baud, carrier)


def test_fewer_than_two_symbols_is_empty():
    import _amr
    import modem
    x = np.random.default_rng(1).normal(0, 0.3, (3, 100)).astype(np.float32)
    for layout in ("row", "lane"):
        pl = _amr.PskPlan("d8psk", 100, 1200, max_streams=3)
        pl.set_layout(layout)
        assert pl.demod_host(x)[0] == [b""] * 3
        outs, sync, softs = pl.demod_soft_host(x)
        assert outs == [b""] * 3 and list(sync) == [-1] * 3 and all(s.size == 0 for s in softs)
    assert modem.d8psk_demodulate(x[0], baud=1200) == b""
    assert modem.d8psk_demodulate_batch(np.zeros((0, 100), np.float32)) == []


def test_device_entries_async_fec_frames_and_gather():
    """What the host layer shares between the kinds, on a d8psk plan: the queued host entry, the
    device entry with the FEC stage, the frame scan of its bytes and a one-rank all-gather of them."""
    import ctypes

    import _amr
    from oracle import oracle
    n = 4097
    baud, carrier = LENGTHS[n]
    x, want = case(n, "f32")
    B = 65
    xb = np.ascontiguousarray(x[:B])
    L = _amr.lib()
    pl = _amr.PskPlan("d8psk", n, baud, carrier, max_streams=B)
    cap = pl.out_cap
    assert cap == 3 * ((n - 5 + 9) // 10 - 1) // 8 + 1
    o, ln, sy = np.zeros((B, cap), np.uint8), np.zeros(B, np.int64), np.zeros(B, np.int64)
    _amr.check(L.amr_psk_demod_host_async(pl.handle, _amr.ptr(xb), _amr.DTYPE_F32, B, n, _amr.ptr(o), cap,
                                          _amr.ptr(ln), _amr.ptr(sy)))
    _amr.check(L.amr_psk_plan_synchronize(pl.handle))
    assert [o[i, :ln[i]].tobytes() for i in range(B)] == [w[0] for w in want[:B]]
    assert list(sy) == [w[2] for w in want[:B]]
    uid = (ctypes.c_uint8 * 128)()
    _amr.check(L.amr_comm_unique_id(uid))
    comm = ctypes.c_void_p()
    with Dev() as d:
        _amr.check(L.amr_comm_create(ctypes.byref(comm), uid, 1, 0, _amr.default_device()))
        d_x, d_out, d_fec = d.put(xb), d.put(np.zeros((B, cap), np.uint8)), d.put(np.zeros((B, cap), np.uint8))
        d_len, d_sync, d_flen = (d.put(np.zeros(B, np.int64)) for _ in range(3))
        d_crc, d_g = d.put(np.zeros(B, np.int32)), d.put(np.zeros((B, cap), np.uint8))
        _amr.check(L.amr_psk_demod_fec_device(pl.handle, d_x, _amr.DTYPE_F32, B, n, d_out, cap, d_len, d_sync,
                                              d_fec, cap, d_flen, d_crc))
        _amr.check(L.amr_allgather(comm, d_out, d_g, B * cap, pl.handle))
        _amr.check(L.amr_psk_plan_synchronize(pl.handle))
        out, g = d.get(d_out, np.zeros((B, cap), np.uint8)), d.get(d_g, np.zeros((B, cap), np.uint8))
        ln2, fl = d.get(d_len, np.zeros(B, np.int64)), d.get(d_flen, np.zeros(B, np.int64))
        fec, crc = d.get(d_fec, np.zeros((B, cap), np.uint8)), d.get(d_crc, np.zeros(B, np.int32))
        _amr.check(L.amr_comm_destroy(comm))
    raws = [out[i, :ln2[i]].tobytes() for i in range(B)]
    assert raws == [w[0] for w in want[:B]] and [g[i, :ln2[i]].tobytes() for i in range(B)] == raws
    for i in range(B):
        dec, ok = oracle.fec_decode(raws[i])
        assert fec[i, :fl[i]].tobytes() == dec and bool(crc[i]) == bool(ok), i
    import tail_cases as tc
    for (cnt, recs), raw in zip(_amr.frame_parse(raws[:8], max_cands=8), raws):
        ref = tc.ref_frame_parse(raw)[0]
        assert cnt == len(ref) and [int(r["status"]) for r in recs] == [w["status"] for w in ref[:8]]


# ---- 3. transmit ------------------------------------------------------------------------
@pytest.mark.parametrize("baud", [19200, 9600, 1200])        # sps 5 (no ramp), 10, 80
def test_modulate_batch_equals_the_restatement(baud):
    import modem
    rng = np.random.default_rng(baud)
    lens = [0, 1, 2, 3, 4, 31, 32, 33, 97]                   # tail padding 0 / 1 / 2 bits, T1's 32-byte edge
    datas = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in lens]
    carrier = {19200: 24000.0, 9600: 12000.0, 1200: 3000.0}[baud]
    refs = [p8.modulate(d, baud, carrier) for d in datas]
    natural = max(r.size for r in refs)
    for n_out in (None, natural - 7 * (96000 // baud) - 3, natural + 37):
        want = np.zeros((len(datas), natural if n_out is None else n_out), np.float32)
        for i, r in enumerate(refs):
            k = min(r.size, want.shape[1])
            want[i, :k] = r[:k]
        got, pcm = modem.modulate_batch("d8psk", datas, baud, carrier, n_out=n_out, pcm=True)
        assert_close(got, want, pcm, (want * np.float32(32767)).astype(np.int16), (baud, n_out))
    one = modem.d8psk_modulate(datas[5], baud, carrier)
    assert_close(one, refs[5], what=(baud, "single"))


def test_modulate_refuses_less_than_one_sample_per_symbol():
    import _amr
    import modem
    with pytest.raises(_amr.AmrError):
        modem.d8psk_modulate(b"abc", baud=200000)


# ---- 4. loopback and the coded chain ----------------------------------------------------
@pytest.mark.parametrize("sigma", [0.0, 0.05])
@pytest.mark.parametrize("baud,carrier", p8.CONFIGS)
def test_loopback_frames_parse(baud, carrier, sigma):
    """GPU modulator -> noise -> GPU demodulator -> frame scan: every frame's payload comes back, CRC valid."""
    import modem
    from test_gpu_loopback import _frames, _payloads, _want_payload
    rng = np.random.default_rng(baud)
    frames = _frames(6, 48, seed=baud)
    x = modem.modulate_batch("d8psk", frames, baud, carrier)
    if sigma:
        x = x + rng.normal(0, sigma, x.shape).astype(np.float32)
    raws = modem.d8psk_demodulate_batch(x, baud, carrier)
    got = _payloads(raws)
    for i, fr in enumerate(frames):
        assert raws[i][:len(fr)] == fr and got[i] == [_want_payload(fr)], (baud, sigma, i)


def test_end_to_end_coded_chain():
    """encode_batch -> d8psk modulate -> noise -> d8psk soft demodulation -> decode_soft_batch returns the
    messages.  9600 Bd on a 12 kHz carrier, 16 messages of 24 bytes, N(0, 0.2^2) on the samples (seed 7): the
    level was picked by running this chain's restatement on the CPU (psk8_cases.modulate -> demod_soft ->
    soft_cases.soft_decode_batch) at 0.1 .. 0.25.  At 0.2 every one of the 16 received codewords has byte
    errors, the uncoded 16-bit sync word is still found in all 16 streams (at 0.25 it is lost in 2 to 4 of
    them: the band-pass is clamped to nearly the whole band at this rate, so the sync, not the code, sets the
    limit) and the soft decoder returns all 16 messages.  The restatement runs here again, so the GPU's soft
    values are checked at this level too."""
    import fec
    import modem
    rng = np.random.default_rng(7)
    msgs = vc.messages(rng, [24] * 16)
    cws = fec.ConvolutionalEncoder().encode_batch(msgs)
    L = len(cws[0])
    assert L == 50 and cws == [vc.encode(m) for m in msgs]
    tx = modem.modulate_batch("d8psk", [b"FB" + c for c in cws], baud=9600, f0=12000.0)
    x = np.zeros((16, tx.shape[1] + 400))
    x[:, 200:200 + tx.shape[1]] = tx
    x = (x + rng.normal(0, 0.2, x.shape)).astype(np.float32)
    outs, softs = modem.d8psk_demodulate_soft_batch(x, baud=9600, carrier=12000.0)
    want = [p8.demod_soft(r, 9600, 12000.0) for r in x]
    assert outs == [w[0] for w in want] and all(np.array_equal(s, w[1]) for s, w in zip(softs, want))
    assert all(o[:2] == b"FB" and len(o) >= 2 + L for o in outs)          # sync found in all
    assert all(o[2:2 + L] != c for o, c in zip(outs, cws))                # and every hard codeword is damaged
    rows = [s[16:16 + 8 * L] for s in softs]
    assert [m for m, _ in sc.soft_decode_batch(rows)] == msgs
    assert fec.ViterbiDecoder().decode_soft_batch(rows) == msgs
