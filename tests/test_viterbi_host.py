"""The K=7 convolutional code and its Viterbi decoder, host side (no GPU): the
numpy restatement in tests/viterbi_cases.py against the reference encoder's
recorded outputs and against brute-force maximum likelihood, the product's
host encoder against the same recordings, and the C ABI's refusals."""
import ctypes

import numpy as np
import pytest

import viterbi_cases as vc

NEW_SYMBOLS = ["amr_conv_encoded_len", "amr_conv_encode_host", "amr_viterbi_work_bytes",
               "amr_viterbi_decode_device", "amr_viterbi_decode_host"]


@pytest.fixture(scope="module", autouse=True)
def product(built_lib):
    """The restatement is only worth testing beside the product it restates:
    every test here needs the library's new entries and fec's new methods."""
    import _amr
    import fec
    L = _amr.lib()
    for name in NEW_SYMBOLS:
        assert name in _amr.EXPORTS and getattr(L, name).argtypes is not None, name
    for cls, name in ((fec.ConvolutionalEncoder, "encode_batch"), (fec.ViterbiDecoder, "decode_ml"),
                      (fec.ViterbiDecoder, "decode_ml_batch")):
        assert callable(getattr(cls, name)), name
    return L


@pytest.fixture(scope="module")
def golden():
    return vc.golden()


def test_restated_encoder_equals_reference_recordings(golden):
    assert len(golden) == 4 * 46
    for kind, msg, cw in golden:
        assert len(cw) == 2 * len(msg) + 2
        assert vc.encode(msg) == cw, (kind, len(msg))
        assert np.array_equal(vc.unpack(cw), vc.encode_bits(msg))
    assert vc.encode(b"") == b"\x00\x00"


def test_product_host_encoder_equals_reference_recordings(golden):
    import fec
    enc = fec.ConvolutionalEncoder()
    for kind, msg, cw in golden:
        if len(msg) <= 255 or kind == "rand":           # the pure-Python loop: the long patterns once is enough
            assert enc.encode(msg) == cw, (kind, len(msg))


def test_stub_decoder_is_still_the_references():
    """ViterbiDecoder.decode stays the reference's stub (fec.py:126-155)."""
    import fec
    cw = vc.encode(b"\xa5\x5a\x01")
    kept = np.unpackbits(np.frombuffer(cw, np.uint8))[:-12][0::2]      # drop 12 bits, keep every second one
    assert fec.ViterbiDecoder().decode(cw) == vc.pack(kept) != b"\xa5\x5a\x01"


def test_clean_codewords_decode_with_metric_zero(golden):
    rand = [(m, c) for k, m, c in golden if k == "rand" and len(m) <= 40]
    assert [len(m) for m, _ in rand] == list(range(41))
    got = vc.decode_batch([c for _, c in rand])
    assert got == [(m, 0) for m, _ in rand]
    pats = [(m, c) for k, m, c in golden if k != "rand" and len(m) <= 40]
    assert vc.decode_batch([c for _, c in pats]) == [(m, 0) for m, _ in pats]


def test_free_distance_is_10():
    assert vc.free_distance() == 10
    # and a codeword of that weight exists among the short messages
    w = vc.codebook_bits(1).sum(axis=1)
    assert w[0] == 0 and w[1:].min() == 10


def test_up_to_four_flips_are_corrected():
    """Half the free distance: <= 4 inverted bits always decode to the message,
    metric = the number of flips, whatever the last byte's high nibble holds."""
    cases = vc.flip_cases(seed=401, count=300)
    assert {k for _, _, k in cases} == {0, 1, 2, 3, 4}
    assert any(rx[-1] >> 4 for _, rx, _ in cases)
    got = vc.decode_batch([rx for _, rx, _ in cases])
    for (msg, rx, k), (dec, metric) in zip(cases, got):
        assert dec == msg and metric == k, (len(msg), k)


def _brute(n, inputs):
    book = vc.codebook_bits(n)                              # [256 ** n][16 n + 12]
    got = vc.decode_batch(inputs)
    several = 0
    for rx, (dec, metric) in zip(inputs, got):
        dist = np.count_nonzero(book != vc.unpack(rx)[None, :], axis=1)
        best = int(dist.min())
        assert metric == best, (n, rx.hex())
        assert dist[int.from_bytes(dec, "big")] == best, (n, rx.hex())       # the decoded message is a minimiser
        assert vc.distance(rx, dec) == best
        several += int(np.count_nonzero(dist == best) > 1)
    return several


def test_brute_force_maximum_likelihood_one_byte():
    rng = np.random.default_rng(11)
    inputs = [rng.integers(0, 256, 4, dtype=np.uint8).tobytes() for _ in range(60)]
    inputs += [bytes(4), b"\xff" * 4, b"\xaa" * 4, b"\x55" * 4]
    assert _brute(1, inputs) >= 1                           # ties between codewords occur: the tie rule is exercised


def test_brute_force_maximum_likelihood_two_bytes():
    rng = np.random.default_rng(12)
    inputs = [rng.integers(0, 256, 6, dtype=np.uint8).tobytes() for _ in range(18)] + [b"\xff" * 6, b"\xaa" * 6]
    assert len(inputs) == 20
    assert _brute(2, inputs) >= 1


def test_high_nibble_of_the_last_byte_is_ignored():
    msg = b"nibble"
    cw = vc.flip(vc.encode(msg), [3, 50])
    want = vc.decode(cw)
    assert want == (msg, 2)
    assert all(vc.decode(vc.set_high_nibble(cw, h)) == want for h in range(16))


def test_length_arithmetic(product):
    L = product
    assert [L.amr_conv_encoded_len(n) for n in (0, 1, 2398, 4799)] == [2, 4, 4798, 9600]
    assert L.amr_conv_encoded_len(-1) < 0
    # 512 bytes per 64 steps of the longest codeword a row holds: T = 4 L - 2 for even L
    for stride, blocks in ((0, 0), (1, 0), (2, 1), (3, 1), (16, 1), (17, 1), (18, 2), (4798, 300), (4799, 300),
                           (9600, 600)):
        assert L.amr_viterbi_work_bytes(stride, 1) == blocks * 512, stride
        assert L.amr_viterbi_work_bytes(stride, 7) == 7 * blocks * 512
    assert L.amr_viterbi_work_bytes(4798, 8192) == 8192 * 300 * 512
    assert L.amr_viterbi_work_bytes(1 << 30, 1) == L.amr_viterbi_work_bytes(1 << 24, 1) == (1 << 20) * 512
    assert L.amr_viterbi_work_bytes(4798, 0) == 0
    assert L.amr_viterbi_work_bytes(-1, 1) < 0 and L.amr_viterbi_work_bytes(10, -1) < 0


def test_decode_device_refusals(product):
    """Bad arguments are refused, with a message, before any device work."""
    import _amr
    L = product
    buf = np.zeros((2, 16), np.uint8)
    out = np.zeros((2, 8), np.uint8)
    ln = np.array([16, 16], np.int64)
    oln = np.zeros(2, np.int64)
    met = np.zeros(2, np.int32)
    work = np.zeros(2 * 512, np.uint8)
    p = _amr.ptr

    def call(d_in=p(buf), in_stride=16, d_len=p(ln), n=2, d_out=p(out), out_stride=8, d_oln=p(oln), d_met=p(met),
             d_work=p(work), wb=1024):
        return L.amr_viterbi_decode_device(None, d_in, in_stride, d_len, n, d_out, out_stride, d_oln, d_met, d_work, wb)

    for kw, word in (({"n": -1}, b"negative"), ({"in_stride": -1}, b"negative"), ({"out_stride": -1}, b"negative"),
                     ({"d_in": None}, b"NULL"), ({"d_len": None}, b"NULL"), ({"d_out": None}, b"NULL"),
                     ({"d_oln": None}, b"NULL"), ({"d_met": None}, b"NULL"),
                     ({"out_stride": 6}, b"out_stride"), ({"d_work": None}, b"work buffer"),
                     ({"wb": 1023}, b"work buffer")):
        assert call(**kw) == _amr.AMR_E_INVALID, kw
        assert word in L.amr_last_error(), (kw, L.amr_last_error())
    assert call(n=0, d_in=None, d_len=None, d_out=None, d_oln=None, d_met=None, d_work=None, wb=0) == _amr.AMR_OK
    assert not out.any() and not oln.any() and not met.any()


def test_decode_host_refusals(product):
    import _amr
    L = product
    buf = np.zeros((3, 16), np.uint8)
    out = np.zeros((3, 8), np.uint8)
    oln = np.zeros(3, np.int64)
    met = np.zeros(3, np.int32)
    p = _amr.ptr

    def call(lens, in_=p(buf), in_stride=16, n=3, out_=p(out), out_stride=8, oln_=p(oln), met_=p(met)):
        ln = np.array(lens, np.int64)
        return L.amr_viterbi_decode_host(in_, in_stride, p(ln), n, out_, out_stride, oln_, met_)

    for bad in (0, 1, 3, 15, 18, -2, (1 << 24) + 2):        # not even, < 2, > in_stride, > 2^24
        assert call([16, 4, bad]) == _amr.AMR_E_INVALID, bad
        msg = L.amr_last_error()
        assert b"stream 2" in msg and str(bad).encode() in msg, msg
    assert call([16, 1, 16]) == _amr.AMR_E_INVALID and b"stream 1" in L.amr_last_error()
    for kw in ({"n": -1}, {"in_stride": -1}, {"out_stride": -1}, {"in_": None}, {"oln_": None}, {"met_": None},
               {"out_": None}, {"out_stride": 6}):
        assert call([16, 16, 16], **kw) == _amr.AMR_E_INVALID, kw
    assert L.amr_viterbi_decode_host(p(buf), 16, None, 3, p(out), 8, p(oln), p(met)) == _amr.AMR_E_INVALID
    assert L.amr_viterbi_decode_host(None, 0, None, 0, None, 0, None, None) == _amr.AMR_OK
    assert not out.any() and not oln.any() and not met.any()


def test_encode_host_refusals(product):
    import _amr
    L = product
    buf = np.zeros((2, 8), np.uint8)
    out = np.zeros((2, 18), np.uint8)
    oln = np.zeros(2, np.int64)
    p = _amr.ptr

    def call(lens, in_=p(buf), in_stride=8, n=2, out_=p(out), out_stride=18, oln_=p(oln)):
        ln = np.array(lens, np.int64)
        return L.amr_conv_encode_host(in_, in_stride, p(ln), n, out_, out_stride, oln_)

    assert call([8, 9]) == _amr.AMR_E_INVALID and b"stream 1" in L.amr_last_error()
    assert call([-1, 8]) == _amr.AMR_E_INVALID and b"stream 0" in L.amr_last_error()
    for kw in ({"n": -1}, {"in_stride": -1}, {"out_stride": -1}, {"in_": None}, {"out_": None}, {"oln_": None},
               {"out_stride": 17}):
        assert call([8, 8], **kw) == _amr.AMR_E_INVALID, kw
    assert L.amr_conv_encode_host(p(buf), 8, None, 2, p(out), 18, p(oln)) == _amr.AMR_E_INVALID
    assert L.amr_conv_encode_host(None, 0, None, 0, None, 0, None) == _amr.AMR_OK
    assert not out.any() and not oln.any()


def test_bad_lengths_are_value_errors_before_any_device_work(product):
    import fec
    dec = fec.ViterbiDecoder()
    for n in (0, 1, 3):
        with pytest.raises(ValueError):
            dec.decode_ml(bytes(n))
    with pytest.raises(ValueError) as e:
        dec.decode_ml_batch([bytes(4), bytes(5)], return_errors=True)
    assert "codeword 1" in str(e.value)


def test_no_gpu_is_an_error_not_a_fallback(product):
    import _amr
    import fec
    if _amr.device_count() > 0:
        return                                              # the GPU suite covers the working path
    with pytest.raises(_amr.AmrError):
        fec.ConvolutionalEncoder().encode_batch([b"abc"])
    with pytest.raises(_amr.AmrError):
        fec.ViterbiDecoder().decode_ml(bytes(8))
    with pytest.raises(_amr.AmrError):
        fec.ViterbiDecoder().decode_ml_batch([bytes(8), bytes(2)], return_errors=True)
    with pytest.raises(_amr.AmrError):
        _amr.conv_encode([b"x"])
    with pytest.raises(_amr.AmrError):
        _amr.viterbi_decode([bytes(4)])
