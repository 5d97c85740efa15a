"""The soft-decision definitions of DESIGN §3g without a GPU: the numpy
restatement in tests/soft_cases.py (the checker of the GPU kernels) against
the hard restatement, a brute-force search of the codebook and the oracle's
demodulators, and the new ABI entries' argument checks."""
import numpy as np
import pytest

import soft_cases as sc
import viterbi_cases as vc

NEW_SYMBOLS = ["amr_psk_demod_soft_host", "amr_psk_demod_soft_device", "amr_psk_soft_host",
               "amr_viterbi_soft_work_bytes", "amr_viterbi_decode_soft_device", "amr_viterbi_decode_soft_host"]
ERASURE_LENGTHS = [0, 1, 7, 8, 31, 72]


@pytest.fixture(scope="module")
def product(built_lib):
    """The restatement is only worth testing beside the product it restates."""
    import _amr
    import fec
    import modem
    L = _amr.lib()
    for name in NEW_SYMBOLS:
        assert name in _amr.EXPORTS and getattr(L, name).argtypes is not None, name
    for name in ("decode_soft", "decode_soft_batch", "soft_from_bytes"):
        assert callable(getattr(fec.ViterbiDecoder, name)), name
    for name in ("qpsk_demodulate_soft", "bpsk_demodulate_soft", "qpsk_demodulate_soft_batch",
                 "bpsk_demodulate_soft_batch"):
        assert callable(getattr(modem, name)), name
    return L


def unit_rows(cws):
    return [sc.from_codeword(c, 1) for c in cws]


def coding_gain_set(seed=7):
    """The coding-gain recipe: 64 messages of 32 bytes, coded bits at +-1 plus N(0, 0.7^2), quantised to int8.
    Returns (messages, soft rows, sliced hard codewords)."""
    rng = np.random.default_rng(seed)
    msgs = vc.messages(rng, [32] * 64)
    rows, hard = [], []
    for m in msgs:
        c = vc.encode_bits(m).astype(np.float64)
        y = (2 * c - 1) + 0.7 * rng.standard_normal(c.size)
        q = np.clip(np.floor(np.abs(y) * 64 + 0.5), 1, 127)
        rows.append(np.where(y > 0, q, -q).astype(np.int8))
        hard.append(vc.pack((y > 0).astype(np.uint8)))
    return msgs, rows, hard


# ---------------------------------------------------------------------------
def test_unit_magnitudes_are_the_hard_decoder(product):
    rx = [r for _, r, _ in vc.flip_cases(11, 300)]
    rx += vc.tie_inputs(seed=9, lengths=[0, 1, 2, 7, 8, 16, 33])
    rx += [r for _, r in vc.noisy(seed=50, lengths=[1, 7, 8, 15, 16, 31, 32, 72, 130], ber=0.05)]
    assert sc.soft_decode_batch(unit_rows(rx)) == vc.decode_batch(rx)


def test_both_row_forms_agree(product):
    rng = np.random.default_rng(21)
    rows = [rng.integers(-128, 128, 16 * n + 12).astype(np.int8) for n in (0, 1, 2, 7, 8, 40)]
    images = [sc.byte_image(r, nibble=int(rng.integers(-128, 128))) for r in rows]
    assert all(im.size % 16 == 0 and im.size == r.size + 4 for im, r in zip(images, rows))
    assert sc.soft_decode_batch(images) == sc.soft_decode_batch(rows)
    mixed = [images[0], rows[1], images[2], rows[3], images[4], rows[5]]
    assert sc.soft_decode_batch(mixed) == sc.soft_decode_batch(rows)


def test_one_byte_messages_against_the_whole_codebook(product):
    """metric = the least disagreement cost over all 256 codewords, and the decoded message attains it."""
    book = vc.codebook_bits(1).astype(bool)                  # [256][28]
    rng = np.random.default_rng(33)
    rows = [rng.integers(-128, 128, 28).astype(np.int8) for _ in range(256)]
    rows[0][:] = 0                                           # all erasures: every codeword costs 0
    rows[1][:] = -128
    got = sc.soft_decode_batch(rows)
    for r, (dec, metric) in zip(rows, got):
        v = sc.bit_stream(r)
        cost = (np.abs(v)[None, :] * (book != (v > 0)[None, :])).sum(axis=1)
        assert metric == cost.min()
        assert len(dec) == 1 and cost[dec[0]] == metric == sc.disagreement(r, dec)


def test_coding_gain_seed_7(product):
    msgs, rows, hard = coding_gain_set(7)
    soft_wrong = sum(d != m for (d, _), m in zip(sc.soft_decode_batch(rows), msgs))
    hard_wrong = sum(d != m for (d, _), m in zip(vc.decode_batch(hard), msgs))
    print(f"seed 7: hard {hard_wrong}/64 wrong, soft {soft_wrong}/64 wrong")
    assert soft_wrong * 4 <= hard_wrong and hard_wrong >= 16


def test_erasures_two_of_three_rate(product):
    """Every fourth value erased (the 2/3 puncturing pattern): clean codewords still decode, at cost 0."""
    msgs = vc.messages(np.random.default_rng(44), ERASURE_LENGTHS)
    rows = []
    for m in msgs:
        r = sc.from_codeword(vc.encode(m), 127)
        r[3::4] = 0
        rows.append(r)
    assert sc.soft_decode_batch(rows) == [(m, 0) for m in msgs]


def psk_golden_cases(golden):
    manifest, inputs = golden
    for c in manifest["cases"]:
        if c["status"] != "ok" or "fsk" in c["fn"]:
            continue
        p = c["params"]
        kind = "bpsk" if c["fn"] == "bpsk_demodulate" else "qpsk"
        yield c["id"], kind, inputs[c["id"]], p.get("baud", p.get("b")), p.get("carrier", 3000.0)


def test_soft_signs_are_the_oracle_bytes_on_the_golden_cases(product, golden):
    from oracle import oracle
    seen = 0
    for cid, kind, x, baud, carrier in psk_golden_cases(golden):
        want = (oracle.qpsk_demodulate if kind == "qpsk" else oracle.bpsk_demodulate)(x, baud, carrier)
        data, soft, _ = sc.demod_soft(kind, x, baud, carrier)
        assert data == want, cid
        assert soft.dtype == np.int8 and soft.size == 8 * len(data), cid
        assert np.packbits(soft > 0).tobytes() == data, cid
        assert not np.any(soft == 0) and not np.any(soft == -128), cid
        seen += 1
    assert seen >= 30


def test_soft_signs_on_noisy_1000_baud_captures(product):
    from oracle import oracle
    rng = np.random.default_rng(3)
    for sigma in (0.3, 0.8):
        msg = b"FB" + rng.integers(0, 256, 6, dtype=np.uint8).tobytes()
        x = oracle.qpsk_modulate(msg, baud=1000)
        x = np.concatenate([np.zeros(500), x, np.zeros(500)]) + sigma * rng.standard_normal(x.size + 1000)
        data, soft, _ = sc.demod_soft("qpsk", x.astype(np.float32), 1000)
        assert data == oracle.qpsk_demodulate(x.astype(np.float32), 1000)
        assert np.packbits(soft > 0).tobytes() == data


def test_magnitude_rule_on_plain_values(product):
    """The rule by hand: on an axis both QPSK bits sit at 127; on a diagonal one bit is at its edge."""
    s = sc.psk_soft("qpsk", np.array([1, 1, 1j, -1j, 1 + 1j], np.complex128))
    # products: 1 (sector 0: 00), 1j (01), -1 (11), then (1 + 1j) * conj(-1j) = -1 + 1j: on the 3pi/4 edge
    assert s[:6].tolist() == [-127, -127, -127, 127, 127, 127]
    assert abs(int(s[6])) == 1 and s[7] == 127
    b = sc.psk_soft("bpsk", np.array([1, 1, -1, 1 + 1j], np.complex128))
    assert b.tolist() == [-127, 127, 64]                     # the last: dr = -1, di = -1 -> r = 0.5 -> floor(64.0)
    z = sc.psk_soft("qpsk", np.array([1, 0, np.nan, 1], np.complex128))
    assert np.all(np.abs(z) == 1)


# ---- the ABI's argument checks (no device work before them) ------------------
def test_soft_work_bytes(product):
    L = product
    assert L.amr_viterbi_soft_work_bytes(-1, 1) < 0 and L.amr_viterbi_soft_work_bytes(1, -1) < 0
    assert L.amr_viterbi_soft_work_bytes(11, 5) == 0
    for nv, blocks in ((12, 1), (16, 1), (27, 1), (28, 1), (128, 1), (140, 2), (16 * 32 + 12, 5)):
        assert L.amr_viterbi_soft_work_bytes(nv, 3) == 3 * 512 * blocks, nv
    assert L.amr_viterbi_soft_work_bytes(1 << 40, 1) == ((sc.MAX_VALS // 2 + 63) // 64) * 512


def test_decode_soft_device_refusals(product):
    import _amr
    L = product
    buf = np.zeros((2, 32), np.int8)
    out = np.zeros((2, 8), np.uint8)
    ln = np.array([28, 28], np.int64)
    oln = np.zeros(2, np.int64)
    met = np.zeros(2, np.int32)
    work = np.zeros(2 * 512, np.uint8)
    p = _amr.ptr

    def call(d_in=p(buf), in_stride=32, in_offset=0, d_len=p(ln), n=2, d_out=p(out), out_stride=8, d_oln=p(oln),
             d_met=p(met), d_work=p(work), wb=1024):
        return L.amr_viterbi_decode_soft_device(None, d_in, in_stride, in_offset, d_len, n, d_out, out_stride, d_oln,
                                                d_met, d_work, wb)

    for kw, word in (({"n": -1}, b"negative"), ({"in_stride": -1}, b"negative"), ({"out_stride": -1}, b"negative"),
                     ({"in_offset": -1}, b"negative"), ({"in_offset": 33}, b"in_offset"),
                     ({"d_in": None}, b"NULL"), ({"d_len": None}, b"NULL"), ({"d_out": None}, b"NULL"),
                     ({"d_oln": None}, b"NULL"), ({"d_met": None}, b"NULL"),
                     ({"out_stride": 0}, b"out_stride"), ({"d_work": None}, b"work buffer"),
                     ({"wb": 1023}, b"work buffer")):
        assert call(**kw) == _amr.AMR_E_INVALID, kw
        assert word in L.amr_last_error(), (kw, L.amr_last_error())
    assert call(n=0, d_in=None, d_len=None, d_out=None, d_oln=None, d_met=None, d_work=None, wb=0) == _amr.AMR_OK
    assert not out.any() and not oln.any() and not met.any()


def test_decode_soft_host_refusals(product):
    import _amr
    L = product
    buf = np.zeros((3, 48), np.int8)
    out = np.zeros((3, 8), np.uint8)
    oln = np.zeros(3, np.int64)
    met = np.zeros(3, np.int32)
    p = _amr.ptr

    def call(lens, in_=p(buf), in_stride=48, in_offset=0, n=3, out_=p(out), out_stride=8, oln_=p(oln), met_=p(met)):
        ln = np.array(lens, np.int64)
        return L.amr_viterbi_decode_soft_host(in_, in_stride, in_offset, p(ln), n, out_, out_stride, oln_, met_)

    for bad in (0, 4, 8, 11, 13, 20, 24, 60, 64, -4, sc.MAX_VALS + 16):   # no row length, past the stride, past the maximum
        assert call([28, 12, bad]) == _amr.AMR_E_INVALID, bad
        msg = L.amr_last_error()
        assert b"stream 2" in msg and str(bad).encode() in msg, msg
    assert call([28, 5, 28]) == _amr.AMR_E_INVALID and b"stream 1" in L.amr_last_error()
    assert call([28, 28, 44], in_offset=8) == _amr.AMR_E_INVALID and b"stream 2" in L.amr_last_error()
    for kw in ({"n": -1}, {"in_stride": -1}, {"out_stride": -1}, {"in_offset": -1}, {"in_offset": 49}, {"in_": None},
               {"oln_": None}, {"met_": None}, {"out_": None}, {"out_stride": 1}):
        assert call([44, 44, 44], **kw) == _amr.AMR_E_INVALID, kw
    assert L.amr_viterbi_decode_soft_host(p(buf), 48, 0, None, 3, p(out), 8, p(oln), p(met)) == _amr.AMR_E_INVALID
    assert L.amr_viterbi_decode_soft_host(None, 0, 0, None, 0, None, 0, None, None) == _amr.AMR_OK
    assert not out.any() and not oln.any() and not met.any()


def test_psk_soft_entries_refuse_bad_arguments(product):
    import _amr
    L = product
    sym = np.zeros((2, 4, 2))
    soft = np.zeros((2, 6), np.int8)
    p = _amr.ptr
    assert L.amr_psk_soft_host(7, p(sym), 2, 4, p(soft)) == _amr.AMR_E_INVALID
    assert L.amr_psk_soft_host(0, p(sym), -1, 4, p(soft)) == _amr.AMR_E_INVALID
    assert L.amr_psk_soft_host(0, p(sym), 2, -1, p(soft)) == _amr.AMR_E_INVALID
    assert L.amr_psk_soft_host(0, None, 2, 4, p(soft)) == _amr.AMR_E_INVALID
    assert L.amr_psk_soft_host(0, p(sym), 2, 4, None) == _amr.AMR_E_INVALID
    assert L.amr_psk_soft_host(0, None, 0, 4, None) == _amr.AMR_OK          # an empty batch
    assert L.amr_psk_soft_host(1, p(sym), 2, 1, p(soft)) == _amr.AMR_OK     # one symbol: no product, nothing written
    assert not soft.any()
    x = np.zeros((1, 64), np.float32)
    o = np.zeros((1, 8), np.uint8)
    ln, sy = np.zeros(1, np.int64), np.zeros(1, np.int64)
    for fn in (L.amr_psk_demod_soft_host, L.amr_psk_demod_soft_device):
        assert fn(None, p(x), 0, 1, 64, p(o), 8, p(ln), p(sy), None, p(soft), 64) == _amr.AMR_E_INVALID
        assert b"NULL" in L.amr_last_error()
        assert fn(None, p(x), 0, -1, 64, p(o), 8, p(ln), p(sy), None, p(soft), 64) == _amr.AMR_E_INVALID
        assert fn(None, p(x), 0, 1, 64, p(o), 8, p(ln), p(sy), None, p(soft), -1) == _amr.AMR_E_INVALID
        assert b"negative" in L.amr_last_error()


def test_python_surface_checks_lengths_before_any_device_work(product):
    import fec
    dec = fec.ViterbiDecoder()
    for n in (0, 4, 8, 11, 20, 24):
        with pytest.raises(ValueError):
            dec.decode_soft(np.zeros(n, np.int8))
    with pytest.raises(ValueError) as e:
        dec.decode_soft_batch([np.zeros(28, np.int8), np.zeros(29, np.int8)], return_metrics=True)
    assert "soft row 1" in str(e.value)
    cw = vc.encode(b"soft")
    s = dec.soft_from_bytes(cw)
    assert s.dtype == np.int8 and np.array_equal(s, sc.from_codeword(cw, 1))
    assert np.array_equal(dec.soft_from_bytes(cw, mag=90), sc.from_codeword(cw, 90))
    for bad in (b"\x00", b"\x00\x00\x00"):
        with pytest.raises(ValueError):
            dec.soft_from_bytes(bad)
    with pytest.raises(ValueError):
        dec.soft_from_bytes(cw, mag=128)
