"""star16 on the GPU: k_slice16 and k_psk_soft16 (star16_kernels.hip),
the AMR_TX_STAR16 kernels (tx_kernels.hip) and the plan / host layer around
them against the numpy restatement in tests/star16_cases.py.  The receive side
is bit-equal to the restatement; the transmit samples are under
test_gpu_tx.assert_close's rule (sin's last ulp)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import psk8_cases as p8
import soft_cases as sc
import star16_cases as s16
import viterbi_cases as vc
from test_gpu_psk8 import boundary_products
from test_gpu_tx import assert_close
from test_gpu_viterbi import Dev

pytestmark = pytest.mark.gpu

B_MAX = 130
LENGTHS = {2110: (19200, 24000.0), 4097: (9600, 12000.0), 9613: (2400, 3000.0)}     # n -> (baud, carrier)
DTYPES = ["f32", "f64", "pcm16", "raw16"]
# products per stream: 8 is the word (k_slice16's unit), 64 a wave's share of the workgroup's 256, 16 and 64
# k_psk_soft16's wave and tile
PRODUCTS = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 67, 255, 256, 257]
STREAMS = [1, 63, 64, 65, 67]
TAIL = 4                     # symbols of silence after a frame (test_star16_host.test_round_trip says why)


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")
    assert _amr.psk_kind("star16") == _amr.PSK_STAR16        # the restatement is only worth testing beside the product


def want_bits(sym):
    return np.stack([s16.slice_bits(r) for r in np.atleast_2d(sym)])


def want_soft(sym):
    return np.stack([s16.soft(r) for r in np.atleast_2d(sym)])


def ring_symbols(rng, B, S):
    """Noisy symbols of both rings at one random scale per stream."""
    z = np.exp(2j * np.pi * rng.uniform(0, 1, (B, S))) * rng.choice([0.5, 1.0], (B, S))
    z = z + 0.08 * (rng.standard_normal((B, S)) + 1j * rng.standard_normal((B, S)))
    return z * np.exp2(rng.integers(-30, 31, (B, 1)))


# ---- 1. the slicer and the soft stage alone -----------------------------------------
def test_slicer_stage_sizes():
    import _amr
    rng = np.random.default_rng(160)
    seen = np.zeros(16, np.int64)
    for nd in PRODUCTS:
        for B in STREAMS:
            sym = ring_symbols(rng, B, nd + 1)
            got = _amr.psk_slice("star16", sym)
            want = want_bits(sym)
            assert got.shape == (B, 4 * nd) and np.array_equal(got, want), (nd, B)
            seen += np.bincount(np.packbits(want.reshape(-1, 4), axis=1, bitorder="big").ravel() >> 4, minlength=16)
    assert seen.min() > 100                                                                # every nibble was decided
    assert _amr.psk_slice("star16", np.ones((3, 1), np.complex128)).shape == (3, 0)       # S = 1: nothing
    assert _amr.psk_soft("star16", np.ones((3, 1), np.complex128)).shape == (3, 0)


def test_soft_stage_sizes():
    import _amr
    rng = np.random.default_rng(161)
    for nd in PRODUCTS:
        for B in (1, 65):
            sym = ring_symbols(rng, B, nd + 1)
            got = _amr.psk_soft("star16", sym)
            assert got.dtype == np.int8 and got.shape == (B, 4 * nd), (nd, B)
            assert np.array_equal(got, want_soft(sym)), (nd, B)
            assert np.array_equal(got > 0, _amr.psk_slice("star16", sym).astype(bool))    # the sign is the hard bit


def fma_pairs():
    """Symbol pairs (s0, s1) whose ring bit an fma in e would flip: s1's energy as two rounded products and a
    rounded sum differs by an ulp from fma(sr, sr, si * si) (form 0) or fma(si, si, sr * sr) (form 1), and
    s0 = (x, 0) has 2 * x * x exactly the smaller of the two, so `e1 > 2 e0` holds for the larger alone.  Found by
    a seeded search on the CPU (a few dozen tries each); each pair also reversed."""
    def fma(a, b, c):
        return float(Fraction(a) * Fraction(b) + Fraction(c))
    out = []
    for form in (0, 1):
        rng = np.random.default_rng(16 + form)
        found = 0
        for _ in range(100000):
            sr, si = (float(v) for v in rng.uniform(0.5, 1.0, 2))
            e_sep = sr * sr + si * si
            e_fma = fma(sr, sr, si * si) if form == 0 else fma(si, si, sr * sr)
            if e_sep == e_fma:
                continue
            lo = min(e_sep, e_fma)
            x = math.sqrt(lo / 2)
            for c in (x, float(np.nextafter(x, 0.0)), float(np.nextafter(x, 1.0))):
                if c * c == lo / 2:
                    a_sep, a_fma = int(e_sep > 2.0 * (c * c)), int(e_fma > 2.0 * (c * c))
                    assert a_sep != a_fma
                    out.append((complex(c, 0.0), complex(sr, si), a_sep))
                    out.append((complex(sr, si), complex(c, 0.0), a_sep))
                    found += 1
                    break
            if found == 4:
                break
        assert found == 4, form
    return out


def ring_edge_pairs():
    """(s0, s1, the ring bit meant): exact ties e1 == 2 e0 and e0 == 2 e1 with one ulp to each side, at 2^+-500
    too (the energies finite), and the fma pairs."""
    pairs = []
    up, dn = float(np.nextafter(2.0, 3.0)), float(np.nextafter(2.0, 1.0))
    for g in (1.0, 2.0 ** -500, 2.0 ** 500, 2.0 ** -37, 3.0):
        ties = [(complex(1, 1), complex(2, 0), 0), (complex(3, 4), complex(5, 5), 0), (complex(0, -1), complex(1, -1), 0),
                (complex(1, 1), complex(up, 0), 1), (complex(1, 1), complex(dn, 0), 0),
                (complex(0, up), complex(2, 2), 0), (complex(0, dn), complex(2, 2), 1),
                (complex(1, 0), complex(1, 0), 0), (complex(1, 0), complex(0, 2), 1)]
        for s0, s1, a in ties:
            pairs.append((g * s0, g * s1, a))
            pairs.append((g * s1, g * s0, a))
    return pairs + fma_pairs()


def test_ring_ties_and_an_fma_that_would_flip_them():
    import _amr
    pairs = ring_edge_pairs()
    sym = np.array([s for p in pairs for s in p[:2]], np.complex128)
    meant = np.array([p[2] for p in pairs])
    nib = s16.nibbles(sym)
    assert np.array_equal(nib[0::2] >> 3, meant) and 20 < meant.sum() < meant.size - 20   # the cases decide what they are meant to
    for B in (1, 2):
        s2 = np.stack([sym] * B)
        bits, soft = _amr.psk_slice("star16", s2), _amr.psk_soft("star16", s2)
        for i in range(B):
            assert np.array_equal(bits[i], s16.slice_bits(sym)), i
            assert np.array_equal(soft[i], s16.soft(sym)), i


def test_boundary_and_special_products():
    """d8psk's eight phase-boundary ties with an ulp to each side, then zeros, denormals, 2^+-1000 (the energies
    overflow or vanish), infinities and NaN in either component, each against the symbol 1."""
    import _amr
    d = boundary_products()
    sym = np.empty(2 * d.size + 1, np.complex128)
    sym[0::2] = 1.0
    sym[1::2] = d
    prod = sc.diff_products(sym)[0::2]
    fin = np.isfinite(d.real) & np.isfinite(d.imag)
    assert np.array_equal(prod[fin], d[fin]) and fin.sum() > 600
    n = 45
    assert set(p8.steps(prod)[:8 * n].tolist()) == {1, 3, 5, 7}          # an exact tie falls to the diagonal sectors
    assert set(p8.steps(prod)[8 * n:16 * n].tolist()) == {0, 2, 4, 6}    # an ulp towards the axis
    e = s16.energies(sym)
    assert np.isinf(e).sum() > 50 and np.isnan(e).sum() > 20 and (e == 0).sum() > 20
    for B in (1, 2):
        s2 = np.stack([sym] * B)
        bits, soft = _amr.psk_slice("star16", s2), _amr.psk_soft("star16", s2)
        for i in range(B):
            assert np.array_equal(bits[i], s16.slice_bits(sym)), i
            assert np.array_equal(soft[i], s16.soft(sym)), i
    assert not np.any(soft == 0) and not np.any(soft == -128)
    assert np.abs(soft[0].astype(np.int64))[3::4].max() <= 75                          # b0 tops out near 74


# ---- 2. full demodulation ---------------------------------------------------------------
def make_batch(n, dt):
    """[B_MAX][n] streams: payloads whose sync word sits 0 .. 3 bits into a nibble, and noise alone."""
    baud, carrier = LENGTHS[n]
    rng = np.random.default_rng(n)
    sps = 96000 // baud
    room = (n // sps - 41) // 2 - 4
    assert room >= 4
    rows = []
    for i in range(B_MAX):
        body = b"FB" + rng.integers(0, 256, room, dtype=np.uint8).tobytes()
        if i % 3 == 2:
            x = np.zeros(n, np.float32)
        else:
            shift = (i // 3) % 4
            bits = np.concatenate([np.zeros(shift, np.uint8), np.unpackbits(np.frombuffer(body, np.uint8)),
                                   np.zeros(8 - shift, np.uint8)])
            w = s16.modulate(np.packbits(bits).tobytes(), baud, carrier)
            x = np.concatenate([w, np.zeros(max(0, n - w.size), np.float32)])[:n]
        rows.append(x + rng.normal(0, 0.05, n))
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
        want = [s16.demod_soft(x[i], baud, carrier, raw_int16=dt == "raw16") for i in range(B_MAX)]
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
        assert all(np.sum((syncs >= 0) & (syncs % 4 == r)) >= 12 for r in range(4)), (n, syncs)
        assert np.sum(syncs < 0) >= 30 and all(len(w[0]) > 0 for w in want), n
        assert all(s16.demod(x, *LENGTHS[n])[0] == w[0] for x, w in zip(case(n, "f32")[0][:4], want))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", list(LENGTHS))
def test_demod_equals_the_restatement(n, dt):
    import _amr
    baud, carrier = LENGTHS[n]
    x, want = case(n, dt)
    for layout, B in (("row", 3), ("lane", 65), ("lane", B_MAX), ("split", 3)):
        pl = _amr.PskPlan("star16", n, baud, carrier, max_streams=B)
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
        pl = _amr.PskPlan("star16", n, baud, carrier, max_streams=B)
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
    outs = modem.star16_demodulate_batch(x[:9], baud, carrier)
    assert outs == [w[0] for w in want[:9]]
    assert modem.star16_demodulate(x[1], baud, carrier) == want[1][0]
    so, sv = modem.star16_demodulate_soft_batch(x[:9], baud, carrier)
    assert so == outs and all(np.array_equal(a, w[1]) for a, w in zip(sv, want))
    d1, s1 = modem.star16_demodulate_soft(x[4], baud, carrier)
    assert d1 == want[4][0] and np.array_equal(s1, want[4][1])
    ragged = [x[0], x[1].astype(np.float64), case(2110, "f32")[0][0]]
    assert modem.demodulate_ragged("star16", ragged[:2], baud, carrier) == [want[0][0], want[1][0]]
    assert modem.demodulate_ragged("star16", ragged[2:], *LENGTHS[2110]) == [case(2110, "f32")[1][0][0]]
    # 16-bit WAV samples, read as pcm / 32768
    pcm = case(n, "pcm16")
    assert modem._pcm16_star16(pcm[0][0], baud, carrier) == pcm[1][0][0]
    # the alias stays the reference's QPSK
    assert np.array_equal(modem.apsk16_modulate(b"FBPC", baud, carrier), modem.qpsk_modulate(b"FBPC", baud, carrier))


def test_fewer_than_two_symbols_is_empty():
    import _amr
    import modem
    x = np.random.default_rng(1).normal(0, 0.3, (3, 100)).astype(np.float32)
    for layout in ("row", "lane"):
        pl = _amr.PskPlan("star16", 100, 1200, max_streams=3)
        pl.set_layout(layout)
        assert pl.demod_host(x)[0] == [b""] * 3
        outs, sync, softs = pl.demod_soft_host(x)
        assert outs == [b""] * 3 and list(sync) == [-1] * 3 and all(s.size == 0 for s in softs)
    assert modem.star16_demodulate(x[0], baud=1200) == b""
    assert modem.star16_demodulate_batch(np.zeros((0, 100), np.float32)) == []


def test_device_entries_async_fec_frames_and_gather():
    """What the host layer shares between the kinds, on a star16 plan: the queued host entry, the
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
    pl = _amr.PskPlan("star16", n, baud, carrier, max_streams=B)
    cap = pl.out_cap
    assert cap == 4 * ((n - 5 + 9) // 10 - 1) // 8 + 1
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
@pytest.mark.parametrize("baud", [19200, 9600, 1200])        # sps 5, 10, 80
def test_modulate_batch_equals_the_restatement(baud):
    import modem
    rng = np.random.default_rng(baud)
    lens = [0, 1, 2, 3, 4, 31, 32, 33, 97]
    datas = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in lens]
    carrier = {19200: 24000.0, 9600: 12000.0, 1200: 3000.0}[baud]
    refs = [s16.modulate(d, baud, carrier) for d in datas]
    natural = max(r.size for r in refs)
    for n_out in (None, natural - 7 * (96000 // baud) - 3, natural + 37):
        want = np.zeros((len(datas), natural if n_out is None else n_out), np.float32)
        for i, r in enumerate(refs):
            k = min(r.size, want.shape[1])
            want[i, :k] = r[:k]
        got, pcm = modem.modulate_batch("star16", datas, baud, carrier, n_out=n_out, pcm=True)
        assert_close(got, want, pcm, (want * np.float32(32767)).astype(np.int16), (baud, n_out))
    one = modem.star16_modulate(datas[5], baud, carrier)
    assert_close(one, refs[5], what=(baud, "single"))
    # both rings are on the air: the inner ring's symbols peak at half the outer's
    peaks = np.abs(refs[8]).reshape(-1, 96000 // baud).max(axis=1)
    assert peaks.max() <= 1.0 and np.sum(peaks < 0.51) > 20 and np.sum(peaks > 0.9) > 20


def test_modulate_refuses_less_than_one_sample_per_symbol():
    import _amr
    import modem
    with pytest.raises(_amr.AmrError, match="star16"):
        modem.star16_modulate(b"abc", baud=200000)


# ---- 4. loopback, gain and the coded chain ----------------------------------------------
@pytest.mark.parametrize("sigma", [0.0, 0.05])
@pytest.mark.parametrize("baud,carrier", s16.CONFIGS)
def test_loopback_frames_parse(baud, carrier, sigma):
    """GPU modulator -> TAIL symbols of silence -> GPU demodulator -> frame scan.  Clean: every frame comes back
    exactly and parses, CRC valid.  Noisy: the GPU's bytes are the restatement's."""
    import modem
    from test_gpu_loopback import _frames, _payloads, _want_payload
    rng = np.random.default_rng(baud)
    frames = _frames(6, 48, seed=baud)
    x = modem.modulate_batch("star16", frames, baud, carrier)
    x = np.concatenate([x, np.zeros((len(frames), TAIL * (96000 // baud)), np.float32)], axis=1)
    if sigma:
        x = x + rng.normal(0, sigma, x.shape).astype(np.float32)
    raws = modem.star16_demodulate_batch(x, baud, carrier)
    if sigma:
        assert raws == [s16.demod(r, baud, carrier)[0] for r in x], (baud, sigma)
        return
    got = _payloads(raws)
    for i, fr in enumerate(frames):
        assert raws[i][:len(fr)] == fr and got[i] == [_want_payload(fr)], (baud, sigma, i)


def test_gain_invariance_on_the_device():
    """A power-of-two gain changes no byte and no sync index; the soft values do not move either."""
    import modem
    baud, carrier = 9600, 12000.0
    rng = np.random.default_rng(1616)
    datas = [b"FBPC" + rng.integers(0, 256, 90, dtype=np.uint8).tobytes() for _ in range(5)]
    x = modem.modulate_batch("star16", datas, baud, carrier).astype(np.float64)
    x = np.concatenate([x, np.zeros((5, TAIL * 10))], axis=1) + rng.normal(0, 0.05, (5, x.shape[1] + TAIL * 10))
    outs, softs = modem.star16_demodulate_soft_batch(x, baud, carrier)
    assert outs == [s16.demod(r, baud, carrier)[0] for r in x] and all(o[:4] == b"FBPC" for o in outs)
    for g in (-40, 40):
        o2, s2 = modem.star16_demodulate_soft_batch(np.ldexp(x, g), baud, carrier)
        assert o2 == outs and all(np.array_equal(a, b) for a, b in zip(s2, softs)), g


CHAIN_SIGMA = 0.15


def test_end_to_end_coded_chain():
    """encode_batch -> star16 modulate -> noise -> star16 soft demodulation -> decode_soft_batch returns the
    messages.  4800 Bd on a 12 kHz carrier, 16 messages of 24 bytes, 200 samples of silence to each side,
    N(0, 0.15^2) on the samples (seed 16).  The level is the largest of 0.2, 0.15, 0.1, 0.05 at which this
    chain's restatement on the CPU (star16_cases.modulate -> demod_soft -> soft_cases.soft_decode_batch, the same
    seed) has byte errors in every received codeword and still returns every message: at 0.2 one of the 16
    streams loses the uncoded sync word (the others hold 6 to 14 wrong bytes of 50); at 0.15 the codewords hold
    4, 5, 5, 2, 2, 5, 2, 1, 5, 3, 6, 4, 4, 4, 3, 2 wrong bytes and all 16 messages come back; at 0.1 seven
    codewords arrive undamaged.  The restatement runs here again, so the GPU's soft values are checked at this
    level too."""
    import fec
    import modem
    rng = np.random.default_rng(16)
    msgs = vc.messages(rng, [24] * 16)
    cws = fec.ConvolutionalEncoder().encode_batch(msgs)
    L = len(cws[0])
    assert L == 50 and cws == [vc.encode(m) for m in msgs]
    tx = modem.modulate_batch("star16", [b"FB" + c for c in cws], baud=4800, f0=12000.0)
    assert_close(tx, np.stack([s16.modulate(b"FB" + c, 4800, 12000.0) for c in cws]), what="chain tx")
    x = np.zeros((16, tx.shape[1] + 400))
    x[:, 200:200 + tx.shape[1]] = tx
    x = (x + rng.normal(0, CHAIN_SIGMA, x.shape)).astype(np.float32)
    outs, softs = modem.star16_demodulate_soft_batch(x, baud=4800, carrier=12000.0)
    want = [s16.demod_soft(r, 4800, 12000.0) for r in x]
    assert outs == [w[0] for w in want] and all(np.array_equal(s, w[1]) for s, w in zip(softs, want))
    assert all(o[:2] == b"FB" and len(o) >= 2 + L for o in outs)          # sync found in all
    assert all(o[2:2 + L] != c for o, c in zip(outs, cws))                # and every hard codeword is damaged
    rows = [s[16:16 + 8 * L] for s in softs]
    assert [m for m, _ in sc.soft_decode_batch(rows)] == msgs
    assert fec.ViterbiDecoder().decode_soft_batch(rows) == msgs
