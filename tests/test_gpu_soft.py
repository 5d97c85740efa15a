"""Soft decisions on the GPU: K4s k_psk_soft (psk_soft_kernels.hip)
and V2 k_viterbi_soft (viterbi_kernels.hip) against the numpy restatement in
tests/soft_cases.py.  Everything is bit-equal to the restatement.

One sentence of the feature's specification does not follow from its own rule
and is checked as the rule has it: a differential product of denormal or 1e300 components has a
finite, non-zero den = |dr| + |di|, so r is an ordinary quotient (127 on an
axis or a diagonal), not magnitude 1.  Magnitude 1 with the slicer's sign is
asserted for the products that make r a NaN: a NaN or infinite component, or
both components zero.  Every value, special or not, equals the restatement."""
import numpy as np
import pytest

import slicer_cases as slc
import soft_cases as sc
import viterbi_cases as vc
from test_gpu_viterbi import Dev
from test_soft_host import coding_gain_set

pytestmark = pytest.mark.gpu

B_MAX = 130
BATCHES = [1, 3, 65, B_MAX]                                  # below a wave, past one group, past two
CONFIGS = {"qpsk1000": ("qpsk", 1000, 9600), "qpsk9600": ("qpsk", 9600, 2400), "bpsk1200": ("bpsk", 1200, 9600)}
DTYPES = ["f32", "f64", "i16"]
CLEAN_LENGTHS = [0, 1, 7, 8, 15, 16, 31, 32, 72, 511, 2398]


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")


# ---- 1. the soft stage alone on crafted symbols -----------------------------------
def check_stage(kind, sym):
    import _amr
    got = _amr.psk_soft(kind, sym)[0]
    want = sc.psk_soft(kind, sym)
    assert got.dtype == np.int8 and np.array_equal(got, want), (kind, np.flatnonzero(got != want)[:8])
    bits = _amr.psk_slice(kind, sym)[0]
    assert np.array_equal(got > 0, bits.astype(bool))        # the sign is K4a's bit
    assert not np.any(got == 0) and not np.any(got == -128)
    return got


@pytest.mark.parametrize("kind", ["qpsk", "bpsk"])
def test_soft_stage_on_edge_symbols(kind):
    sym = slc.symbols_for(slc.edge_diffs())
    got = check_stage(kind, sym)
    d = sc.diff_products(sym)
    bad = ~np.isfinite(d.real) | ~np.isfinite(d.imag) | ((d.real == 0) & (d.imag == 0))
    assert bad.sum() > 50
    mag = np.abs(got.astype(np.int64))
    mag = mag.reshape(-1, 2) if kind == "qpsk" else mag[:, None]
    assert np.all(mag[bad] == 1)                             # with the slicer's sign: check_stage
    assert mag.max() == 127


@pytest.mark.parametrize("kind", ["qpsk", "bpsk"])
def test_soft_stage_on_near_tie_symbols(kind):
    if kind == "qpsk" and not slc.numpy_is_fixture_host():
        pytest.skip("numpy's arctan2 at an ulp-tie is the reference's only on the fixtures' host (as test_gpu_slicer)")
    got = check_stage(kind, slc.symbols_for(slc.near_tie_diffs(20000)))
    if kind == "qpsk":                                       # on a diagonal one bit sits at its edge, the other is sure
        pairs = np.abs(got.astype(np.int64)).reshape(-1, 2)[0::2]       # the products d themselves (not 1 * conj(d))
        assert np.all(pairs.min(axis=1) == 1) and np.all(pairs.max(axis=1) == 127)


def test_soft_stage_batch_and_odd_sizes():
    """Streams past one group of 64, symbol counts off the 64-product tile and the 16-product word."""
    import _amr
    rng = np.random.default_rng(8)
    for kind, B, S in (("qpsk", 67, 131), ("bpsk", 3, 200), ("qpsk", 1, 2), ("bpsk", 2, 34), ("qpsk", 2, 1)):
        sym = rng.standard_normal((B, S)) + 1j * rng.standard_normal((B, S))
        got = _amr.psk_soft(kind, sym)
        assert got.shape == (B, (S - 1) * (2 if kind == "qpsk" else 1))
        for i in range(B):
            assert np.array_equal(got[i], sc.psk_soft(kind, sym[i])), (kind, B, S, i)


# ---- 2. / 3. demodulation with soft output ------------------------------------------
def make_batch(kind, baud, n, dt):
    """[B_MAX][n] streams: payloads whose sync word sits at an even and at an odd bit offset, and
    noise alone (no sync), each row with its own noise."""
    import synth
    rng = np.random.default_rng(baud + (0 if kind == "qpsk" else 7))
    sps = 96000 // baud
    room = (n // sps - (40 if kind == "qpsk" else 80)) * (2 if kind == "qpsk" else 1) // 8 - 3
    assert room >= 0
    wave = synth.qpsk_waveform if kind == "qpsk" else synth.bpsk_waveform
    rows = []
    for i in range(B_MAX):
        body = rng.integers(0, 256, room, dtype=np.uint8).tobytes()
        if i % 3 == 0:
            x = synth.fit(wave(b"FB" + body, baud), n)
        elif i % 3 == 1:                                     # one bit later: 0 FB... shifted through the bytes
            bits = np.concatenate([[0], np.unpackbits(np.frombuffer(b"FB" + body, np.uint8)), np.zeros(7, np.uint8)])
            x = synth.fit(wave(np.packbits(bits).tobytes(), baud), n)
        else:
            x = np.zeros(n, np.float32)
        rows.append(x + rng.normal(0, 0.25, n))
    x = np.stack(rows)
    if dt == "i16":
        return np.round(np.clip(x, -4, 4) * 8000).astype(np.int16)       # raw values, not PCM
    return x.astype(np.float32 if dt == "f32" else np.float64)


_cases = {}


def case(cfg, dt):
    """(x, [(bytes, soft, sync)] from the restatement), computed once per module."""
    if (cfg, dt) not in _cases:
        kind, baud, n = CONFIGS[cfg]
        x = make_batch(kind, baud, n, dt)
        want = [sc.demod_soft(kind, x[i], baud, raw_int16=True) for i in range(B_MAX)]
        _cases[cfg, dt] = (x, want)
    return _cases[cfg, dt]


def run_soft(pl, x):
    import _amr
    return pl.demod_soft_host(x) if _amr.is_kernel_dtype(x.dtype) else pl.demod_soft_host_raw(x)


def check_soft(got, want, tag):
    outs, sync, softs = got
    assert len(outs) == len(softs) == len(want)
    for i, (data, soft, sy) in enumerate(want):
        assert outs[i] == data and sync[i] == sy, (tag, i)
        assert softs[i].dtype == np.int8 and np.array_equal(softs[i], soft), (tag, i)
        assert np.packbits(softs[i] > 0).tobytes() == outs[i], (tag, i)      # the invariant
        assert not np.any(softs[i] == 0) and not np.any(softs[i] == -128), (tag, i)


def test_the_cases_hold_what_they_should():
    """At 1000 baud the sync word is found, at even and at odd bit offsets, and the noise rows have none.
    The reference's demodulators do not recover their own modulation at 9600 baud QPSK / 1200 baud BPSK
    on a 3 kHz carrier, so those batches are all streams without sync (bits from 0)."""
    for cfg in CONFIGS:
        _, want = case(cfg, "f32")
        syncs = np.array([w[2] for w in want])
        if cfg == "qpsk1000":
            assert np.sum((syncs >= 0) & (syncs % 2 == 1)) > 20 and np.sum((syncs >= 0) & (syncs % 2 == 0)) > 20
        assert np.sum(syncs < 0) > 20, cfg
        assert all(len(w[0]) > 0 for w in want)


@pytest.mark.parametrize("layout", ["row", "lane"])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_demod_soft_equals_the_restatement(cfg, dt, layout):
    import _amr
    kind, baud, n = CONFIGS[cfg]
    x, want = case(cfg, dt)
    for B in BATCHES:
        pl = _amr.PskPlan(kind, n, baud, max_streams=B)
        pl.set_layout(layout)
        check_soft(run_soft(pl, x[:B]), want[:B], (cfg, dt, layout, B))
    # the layout asked for is one the plan runs: a hard call on the last plan reports it, with the same bytes
    hard = pl.demod_host(x) if _amr.is_kernel_dtype(x.dtype) else pl.demod_host_raw(x)
    assert pl.last_layout() == layout and hard[0] == [w[0] for w in want]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_bytes_and_sync_are_the_hard_path(cfg, dt):
    import _amr
    import modem
    kind, baud, n = CONFIGS[cfg]
    x, _ = case(cfg, dt)
    pl = _amr.PskPlan(kind, n, baud, max_streams=B_MAX)
    hard, hsync = pl.demod_host(x) if _amr.is_kernel_dtype(x.dtype) else pl.demod_host_raw(x)
    outs, sync, _ = run_soft(pl, x)
    assert outs == hard and np.array_equal(sync, hsync)
    batch = modem.qpsk_demodulate_batch if kind == "qpsk" else modem.bpsk_demodulate_batch
    soft_batch = modem.qpsk_demodulate_soft_batch if kind == "qpsk" else modem.bpsk_demodulate_soft_batch
    one = modem.qpsk_demodulate_soft if kind == "qpsk" else modem.bpsk_demodulate_soft
    mo, ms = soft_batch(x, baud)
    assert mo == batch(x, baud) == hard
    d1, s1 = one(x[1], baud)
    assert d1 == hard[1] and np.array_equal(s1, ms[1])


def test_fewer_than_two_symbols_is_empty():
    import _amr
    import modem
    x = np.random.default_rng(1).normal(0, 0.3, (3, 60)).astype(np.float32)
    for layout in ("row", "lane"):
        pl = _amr.PskPlan("qpsk", 60, 1000, max_streams=3)
        pl.set_layout(layout)
        outs, sync, softs = pl.demod_soft_host(x)
        assert outs == [b""] * 3 and list(sync) == [-1] * 3 and all(s.size == 0 and s.dtype == np.int8 for s in softs)
    assert modem.qpsk_demodulate_soft(x[0], baud=1000)[0] == b""
    assert modem.qpsk_demodulate_soft_batch(np.zeros((0, 60), np.float32), baud=1000) == ([], [])


def test_a_split_plan_runs_soft_on_exact_symbols_and_stays_split():
    import _amr
    import synth
    n, baud, B = 48000, 9600, 2
    x = synth.qpsk_batch(B, n, baud, seed=4, distinct=B)
    want = [sc.demod_soft("qpsk", x[i], baud) for i in range(B)]
    pl = _amr.PskPlan("qpsk", n, baud, max_streams=B)
    pl.set_layout("split")
    hard = pl.demod_host(x)
    assert pl.last_layout() == "split"
    check_soft(pl.demod_soft_host(x), want, "split")
    assert pl.last_layout() == "split"                       # the soft call leaves the bookkeeping alone
    again = pl.demod_host(x)
    assert pl.last_layout() == "split" and again[0] == hard[0] == [w[0] for w in want]


def test_device_entry_writes_only_the_streams_values():
    """amr_psk_demod_soft_device: rows pre-poisoned, a stride wider than it must be."""
    import _amr
    kind, baud, n = CONFIGS["qpsk9600"]
    x, want = case("qpsk9600", "f32")
    B = 5
    pl = _amr.PskPlan(kind, n, baud, max_streams=B)
    cap = pl.out_cap
    stride = 8 * cap + 13
    soft = np.full((B, stride), 0x55, np.int8)
    with Dev() as d:
        d_x, d_out = d.put(np.ascontiguousarray(x[:B])), d.put(np.zeros((B, cap), np.uint8))
        d_len, d_sync, d_soft = d.put(np.zeros(B, np.int64)), d.put(np.zeros(B, np.int64)), d.put(soft)
        args = (pl.handle, d_x, _amr.DTYPE_F32, B, n, d_out, cap, d_len, d_sync, None, d_soft)
        assert d.L.amr_psk_demod_soft_device(*args, 8 * cap - 1) == _amr.AMR_E_INVALID
        assert b"soft_stride" in d.L.amr_last_error()
        d.a.check(d.L.amr_psk_demod_soft_device(*args, stride))
        d.a.check(d.L.amr_psk_plan_synchronize(pl.handle))
        ln = d.get(d_len, np.zeros(B, np.int64))
        out = d.get(d_out, np.zeros((B, cap), np.uint8))
        soft = d.get(d_soft, soft)
    for i in range(B):
        data, sv, _ = want[i]
        assert out[i, :ln[i]].tobytes() == data and np.array_equal(soft[i, :8 * ln[i]], sv), i
        assert np.all(soft[i, 8 * ln[i]:] == 0x55), i


# ---- 4. the soft-input decoder ---------------------------------------------------
def gpu_decode(rows):
    import fec
    outs, mets = fec.ViterbiDecoder().decode_soft_batch(rows, return_metrics=True)
    assert len(outs) == len(mets) == len(rows)
    return list(zip(outs, mets))


def test_clean_codewords_in_both_forms():
    msgs = vc.messages(np.random.default_rng(5), CLEAN_LENGTHS)
    rows = [sc.from_codeword(vc.encode(m), 127) for m in msgs]
    assert gpu_decode(rows) == [(m, 0) for m in msgs]
    assert gpu_decode([sc.byte_image(r, nibble=-128) for r in rows]) == [(m, 0) for m in msgs]
    import fec
    dec = fec.ViterbiDecoder()
    assert dec.decode_soft(rows[4]) == msgs[4] and dec.decode_soft(rows[0]) == b""
    assert dec.decode_soft_batch([]) == []


def test_coding_gain_set_equals_the_restatement():
    msgs, rows, _ = coding_gain_set(7)
    got = gpu_decode(rows)
    assert got == sc.soft_decode_batch(rows)
    assert sum(d != m for (d, _), m in zip(got, msgs)) == 0


def test_random_rows_and_large_metrics_equal_the_restatement():
    """Tie-dense, saturating rows (0 and -128 among them) in both forms, a saturated row far from every
    codeword (a path metric past 16 bits), and the complement of a 4799-byte codeword at +-127, the
    longest row here (its metric stays small: the complement of a codeword of this code is, away from
    the ends, the codeword of the complemented message)."""
    rng = np.random.default_rng(61)
    rows = []
    for n in (0, 1, 2, 7, 8, 16, 33, 72, 130):
        r = rng.integers(-128, 128, 16 * n + 12).astype(np.int8)
        r[rng.random(r.size) < 0.1] = 0
        r[rng.random(r.size) < 0.05] = -128
        rows += [r, sc.byte_image(rng.choice(np.array([-128, -1, 0, 1, 127], np.int8), r.size), nibble=77)]
    rows.append(np.zeros(16 * 9 + 12, np.int8))                  # all erasures: all ties, metric 0
    rows.append(np.full(16 * 9 + 12, -128, np.int8))
    rows.append(rng.choice(np.array([-128, 127], np.int8), 16 * 511 + 12))   # far from every codeword, saturated
    big = vc.encode(vc.messages(rng, [4799])[0])
    rows.append((-sc.from_codeword(big, 127)).astype(np.int8))
    want = sc.soft_decode_batch(rows)
    got = gpu_decode(rows)
    assert got == want
    print("metrics: random +-127 row of 511 bytes", want[-2][1], "complemented 4799-byte codeword", want[-1][1])
    assert want[-2][1] > 1 << 16                                 # path metrics far past 16 bits
    for r, (dec, metric) in zip(rows, got):
        assert metric == sc.disagreement(r, dec)


def test_erasure_pattern_two_of_three():
    msgs = vc.messages(np.random.default_rng(44), [0, 1, 7, 8, 31, 72])
    rows = []
    for m in msgs:
        r = sc.from_codeword(vc.encode(m), 127)
        r[3::4] = 0
        rows.append(r)
    assert gpu_decode(rows) == [(m, 0) for m in msgs]


def test_unit_magnitudes_equal_the_hard_decoder():
    import fec
    dec = fec.ViterbiDecoder()
    rx = [r for _, r in vc.noisy(seed=50, lengths=[1, 7, 8, 15, 16, 31, 32, 72, 130, 511], ber=0.05)]
    rx += vc.tie_inputs(seed=9, lengths=[0, 1, 2, 7, 8, 16, 33])
    hard = dec.decode_ml_batch(rx, return_errors=True)
    soft = dec.decode_soft_batch([dec.soft_from_bytes(r) for r in rx], return_metrics=True)
    assert soft == hard


@pytest.mark.parametrize("batch", [1, 3, 4, 5, 257])
def test_batch_sizes_with_mixed_lengths_and_forms(batch):
    rng = np.random.default_rng(3000 + batch)
    lengths = rng.integers(0, 41, batch)
    lengths[rng.integers(0, batch)] = 0
    rows = []
    for i, n in enumerate(lengths):
        msg = rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()
        y = (2.0 * vc.encode_bits(msg) - 1) + 0.6 * rng.standard_normal(16 * int(n) + 12)
        r = np.clip(np.round(y * 50), -128, 127).astype(np.int8)
        rows.append(sc.byte_image(r, nibble=int(rng.integers(-128, 128))) if i % 2 else r)
    assert gpu_decode(rows) == sc.soft_decode_batch(rows)


def device_decode(rows, lens, in_stride, in_offset, out_stride, pad=0x5A, poison=0xEE):
    n = len(rows)
    buf = np.full((n, in_stride), pad, np.int8)
    for i, r in enumerate(rows):
        buf[i, in_offset:in_offset + len(r)] = r
    out = np.full((n, out_stride), poison, np.uint8)
    with Dev() as d:
        wb = int(d.L.amr_viterbi_soft_work_bytes(in_stride, n))
        assert wb >= 0
        d_in, d_len = d.put(buf), d.put(np.asarray(lens, np.int64))
        d_out, d_oln, d_met = d.put(out), d.put(np.full(n, -7, np.int64)), d.put(np.full(n, -7, np.int32))
        d_work = d.put(np.zeros(max(wb, 1), np.uint8))
        d.a.check(d.L.amr_viterbi_decode_soft_device(None, d_in, in_stride, in_offset, d_len, n, d_out, out_stride,
                                                     d_oln, d_met, d_work, wb))
        d.a.check(d.L.amr_device_synchronize())
        return d.get(d_out, out), d.get(d_oln, np.zeros(n, np.int64)), d.get(d_met, np.zeros(n, np.int32))


def noisy_rows(seed, lengths):
    rng = np.random.default_rng(seed)
    rows = []
    for n in lengths:
        msg = rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()
        y = (2.0 * vc.encode_bits(msg) - 1) + 0.6 * rng.standard_normal(16 * int(n) + 12)
        rows.append(np.clip(np.round(y * 50), -128, 127).astype(np.int8))
    return rows


@pytest.mark.parametrize("in_offset", [0, 16])
def test_device_entry_offsets_and_buffer_edges(in_offset):
    lengths = [0, 1, 8, 9, 40, 23]
    rows = noisy_rows(31, lengths)
    rows = [sc.byte_image(r, nibble=99) if i % 2 else r for i, r in enumerate(rows)]
    want = sc.soft_decode_batch(rows)
    in_stride, out_stride = in_offset + 16 * 40 + 16 + 13, 40 + 9
    out, oln, met = device_decode(rows, [len(r) for r in rows], in_stride, in_offset, out_stride)
    for i, (dec, metric) in enumerate(want):
        assert oln[i] == len(dec) and met[i] == metric, i
        assert out[i, :oln[i]].tobytes() == dec
        assert np.all(out[i, oln[i]:] == 0xEE)               # nothing past out_len is written


# ---- 5. bad rows --------------------------------------------------------------------
def test_device_entry_isolates_bad_lengths():
    in_stride, out_stride = 16 * 16 + 12 + 6, 20
    rows = noisy_rows(32, [16, 3, 0, 16, 7, 16, 1, 16, 16, 2, 16])
    lens = [len(r) for r in rows]
    bad = {1: 4, 3: 8, 5: in_stride + 10, 7: sc.MAX_VALS + 16, 9: 16 * 2 + 4}     # % 16 in {4, 8}, past the stride, past the maximum
    assert (in_stride + 10) % 16 == 12
    for i, v in bad.items():
        lens[i] = v
    out, oln, met = device_decode(rows, lens, in_stride, 0, out_stride)
    good = [i for i in range(len(rows)) if i not in bad]
    want = sc.soft_decode_batch([rows[i] for i in good])
    for i, (dec, metric) in zip(good, want):
        assert oln[i] == len(dec) and met[i] == metric and out[i, :oln[i]].tobytes() == dec, i
        assert np.all(out[i, oln[i]:] == 0xEE)
    for i in bad:
        assert oln[i] == 0 and met[i] == -1 and np.all(out[i] == 0xEE), i


def test_host_entry_raises_for_the_same():
    import _amr
    import fec
    dec = fec.ViterbiDecoder()
    good = np.ones(28, np.int8)
    for n in (4, 8, 36, 40, sc.MAX_VALS + 16):
        with pytest.raises(ValueError) as e:
            dec.decode_soft_batch([good, np.ones(n, np.int8)])
        assert "soft row 1" in str(e.value)
    buf = np.ones((2, 48), np.int8)
    out, oln, met = np.zeros((2, 4), np.uint8), np.zeros(2, np.int64), np.zeros(2, np.int32)
    for n in (4, 8, 60):                                     # 60: a row length, but past the stride
        ln = np.array([28, n], np.int64)
        rc = _amr.lib().amr_viterbi_decode_soft_host(_amr.ptr(buf), 48, 0, _amr.ptr(ln), 2, _amr.ptr(out), 4,
                                                     _amr.ptr(oln), _amr.ptr(met))
        assert rc == _amr.AMR_E_INVALID and b"stream 1" in _amr.lib().amr_last_error()


# ---- 6. end to end ------------------------------------------------------------------
def test_end_to_end_soft_demodulation_into_the_soft_decoder():
    """modulate -> noise -> soft demodulation -> soft decode, the decoder reading the demodulator's rows
    as they are (past the 16 sync values, a codeword's byte image)."""
    import fec
    import modem
    rng = np.random.default_rng(3)
    msgs = vc.messages(rng, [40] * 24)
    enc = fec.ConvolutionalEncoder()
    cws = enc.encode_batch(msgs)
    L = len(cws[0])
    assert L == 82
    tx = modem.modulate_batch("qpsk", [b"FB" + c for c in cws], baud=1000)
    x = np.zeros((24, tx.shape[1] + 1000))
    x[:, 500:500 + tx.shape[1]] = tx
    x = (x + rng.normal(0, 0.5, x.shape)).astype(np.float32)
    outs, softs = modem.qpsk_demodulate_soft_batch(x, baud=1000)
    assert all(o[:2] == b"FB" and len(o) >= 2 + L for o in outs)          # sync found in all
    dec = fec.ViterbiDecoder()
    got = dec.decode_soft_batch([s[16:16 + 8 * L] for s in softs])
    assert got == msgs
    assert dec.decode_ml_batch([o[2:2 + L] for o in outs]) == msgs        # the pieces meet; no gain is claimed here
