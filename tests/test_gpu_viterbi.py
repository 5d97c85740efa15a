"""The K=7 convolutional code on the GPU (viterbi_kernels.hip): k_conv_encode
against the reference encoder's recorded outputs, k_viterbi against the numpy
restatement in tests/viterbi_cases.py.  Decoded bytes AND metrics are bit-equal
to the restatement everywhere -- also where the decode is wrong, and on inputs
dense in metric ties, which only the strict-less tie rule makes unique."""
import ctypes

import numpy as np
import pytest

import viterbi_cases as vc

pytestmark = pytest.mark.gpu

CLEAN_LENGTHS = [0, 1, 7, 8, 15, 16, 31, 32, 72, 511, 2398, 4799]    # T = 62 at 7, 70 at 8: across a 64-step block
NOISY_LENGTHS = [1, 7, 8, 15, 16, 31, 32, 72, 130, 511, 3, 64]


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")


@pytest.fixture(scope="module")
def golden():
    return vc.golden()


def gpu_decode(cws):
    import fec
    outs, errs = fec.ViterbiDecoder().decode_ml_batch(cws, return_errors=True)
    assert len(outs) == len(errs) == len(cws)
    return list(zip(outs, errs))


class Dev:
    """Device buffers for the *_device entry, freed on exit."""

    def __enter__(self):
        import _amr
        self.a, self.L, self.bufs = _amr, _amr.lib(), []
        _amr.check(self.L.amr_set_device(_amr.default_device()))
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.L.amr_free(p)

    def put(self, arr):
        p = ctypes.c_void_p()
        self.a.check(self.L.amr_malloc(ctypes.byref(p), max(1, arr.nbytes)))
        self.bufs.append(p)
        if arr.nbytes:
            self.a.check(self.L.amr_memcpy_h2d(p, self.a.ptr(arr), arr.nbytes))
        return p

    def get(self, p, arr):
        if arr.nbytes:
            self.a.check(self.L.amr_memcpy_d2h(self.a.ptr(arr), p, arr.nbytes))
        return arr


def device_decode(rows, lens, in_stride, out_stride, pad=0xA5, poison=0xEE):
    """amr_viterbi_decode_device on rows padded with `pad` to in_stride, the
    output pre-filled with `poison`: (out [n][out_stride], out_len, metric)."""
    n = len(rows)
    buf = np.full((n, in_stride), pad, np.uint8)
    for i, r in enumerate(rows):
        buf[i, :len(r)] = np.frombuffer(r, np.uint8)
    out = np.full((n, out_stride), poison, np.uint8)
    with Dev() as d:
        wb = int(d.L.amr_viterbi_work_bytes(in_stride, n))
        assert wb >= 0
        d_in, d_len = d.put(buf), d.put(np.asarray(lens, np.int64))
        d_out, d_oln, d_met = d.put(out), d.put(np.full(n, -7, np.int64)), d.put(np.full(n, -7, np.int32))
        d_work = d.put(np.zeros(max(wb, 1), np.uint8))
        d.a.check(d.L.amr_viterbi_decode_device(None, d_in, in_stride, d_len, n, d_out, out_stride, d_oln, d_met,
                                                 d_work, wb))
        d.a.check(d.L.amr_device_synchronize())
        return d.get(d_out, out), d.get(d_oln, np.zeros(n, np.int64)), d.get(d_met, np.zeros(n, np.int32))


# ---------------------------------------------------------------------------
def test_encode_batch_equals_reference_recordings(golden):
    import fec
    enc = fec.ConvolutionalEncoder()
    msgs = [m for _, m, _ in golden]
    assert len({len(m) for m in msgs}) == 46                # one ragged launch: lengths 0 .. 2398 together
    got = enc.encode_batch(msgs)
    for (kind, msg, cw), g in zip(golden, got):
        assert g == cw, (kind, len(msg))
    assert enc.encode_batch([]) == []
    assert enc.encode_batch([b""]) == [b"\x00\x00"]
    assert enc.encode_batch([msgs[-1]]) == [golden[-1][2]]  # alone: a batch of one


def test_ragged_encode_equals_host_encoder():
    import fec
    enc = fec.ConvolutionalEncoder()
    msgs = vc.messages(np.random.default_rng(77), [5, 0, 1, 300, 2, 0, 129, 64, 7])
    assert enc.encode_batch(msgs) == [enc.encode(m) for m in msgs] == [vc.encode(m) for m in msgs]


def test_clean_codewords_decode_exactly():
    """A clean codeword's nearest codeword is itself: (message, 0) with no need of the restatement."""
    msgs = vc.messages(np.random.default_rng(5), CLEAN_LENGTHS)
    cws = [vc.encode(m) for m in msgs]
    assert [len(c) for c in cws][-2:] == [4798, 9600]
    assert gpu_decode(cws) == [(m, 0) for m in msgs]
    import fec
    assert fec.ViterbiDecoder().decode_ml(cws[4]) == msgs[4]
    assert fec.ViterbiDecoder().decode_ml(cws[0]) == b""


def test_up_to_four_flips_are_corrected():
    cases = vc.flip_cases(seed=402, count=300)
    got = gpu_decode([rx for _, rx, _ in cases])
    assert got == [(msg, k) for msg, _, k in cases]


@pytest.mark.parametrize("ber", [0.02, 0.05, 0.12])
def test_noisy_codewords_equal_the_restatement(ber):
    lengths = NOISY_LENGTHS + ([2398] if ber == 0.02 else [])
    cases = vc.noisy(seed=int(ber * 1000), lengths=lengths, ber=ber)
    rx = [r for _, r in cases]
    want = vc.decode_batch(rx)
    got = gpu_decode(rx)
    assert got == want
    if ber == 0.12:                                         # beyond the code: wrong decodes, still the same wrong decodes
        assert any(dec != msg for (dec, _), (msg, _) in zip(got, cases))
    for r, (dec, metric) in zip(rx, got):
        assert metric == vc.distance(r, dec)


def test_tie_dense_inputs_equal_the_restatement():
    rx = vc.tie_inputs(seed=9, lengths=[0, 1, 2, 7, 8, 16, 33, 72])
    want = vc.decode_batch(rx)
    got = gpu_decode(rx)
    assert got == want
    for r, (dec, metric) in zip(rx, got):
        assert len(dec) == len(r) // 2 - 1 and metric == vc.distance(r, dec)


@pytest.mark.parametrize("batch", [1, 3, 4, 5, 257])
def test_batch_sizes_with_mixed_lengths(batch):
    """4 codewords per workgroup: batches below, at and past it, zero-byte messages among them."""
    rng = np.random.default_rng(1000 + batch)
    lengths = rng.integers(0, 41, batch)
    lengths[rng.integers(0, batch)] = 0
    cases = vc.noisy(seed=2000 + batch, lengths=lengths, ber=0.05)
    rx = [r for _, r in cases]
    assert gpu_decode(rx) == vc.decode_batch(rx)


def test_buffer_edges_on_the_device_entry():
    """in_stride > L with the padding 0xA5, the output pre-poisoned, the last byte's high nibble set."""
    lengths = [0, 1, 8, 9, 40, 23]
    cases = vc.noisy(seed=31, lengths=lengths, ber=0.04)
    rx = [vc.set_high_nibble(r, 0xF) for _, r in cases]
    want = vc.decode_batch(rx)
    assert want == vc.decode_batch([vc.set_high_nibble(r, 0) for r in rx])
    in_stride, out_stride = 2 * 40 + 2 + 13, 40 + 9
    out, oln, met = device_decode(rx, [len(r) for r in rx], in_stride, out_stride)
    for i, (dec, metric) in enumerate(want):
        assert oln[i] == len(dec) and met[i] == metric
        assert out[i, :oln[i]].tobytes() == dec
        assert np.all(out[i, oln[i]:] == 0xEE)              # nothing past out_len is written


def test_device_entry_isolates_bad_lengths():
    """The device entry reads the lengths in HBM: a bad one costs only its own row."""
    in_stride, out_stride = 34, 20
    cases = vc.noisy(seed=32, lengths=[16, 3, 0, 16, 7, 16, 1, 16, 16], ber=0.03)
    rx = [r for _, r in cases]
    lens = [len(r) for r in rx]
    bad = {1: 0, 3: 1, 5: 3, 7: in_stride + 2}
    for i, v in bad.items():
        lens[i] = v
    out, oln, met = device_decode(rx, lens, in_stride, out_stride)
    good = [i for i in range(len(rx)) if i not in bad]
    want = vc.decode_batch([rx[i] for i in good])
    for i, (dec, metric) in zip(good, want):
        assert oln[i] == len(dec) and met[i] == metric and out[i, :oln[i]].tobytes() == dec, i
        assert np.all(out[i, oln[i]:] == 0xEE)
    for i in bad:
        assert oln[i] == 0 and met[i] == -1 and np.all(out[i] == 0xEE), i
