"""The Reed-Solomon code on the GPU (rs_kernels.hip): k_rs_encode and k_rs_decode
against the numpy restatement in tests/rs_cases.py.  Bytes, out_len, corrected
and failed are bit-equal to the restatement everywhere -- also where a block is
beyond the code and fails or lands on another codeword."""
import ctypes

import numpy as np
import pytest

import rs_cases as rc

pytestmark = pytest.mark.gpu

NSYMS = [2, 3, 10, 32, 33, 63, 64]                          # 32 | 33: two half-wave groups of syndrome chains, or one
LAST_BLOCKS = [None, 63, 64, 65, 128, 254, 255]             # None: nsym + 1, the shortest last block


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")


def gpu_decode(datas, nsym, I=1, erasures=None):
    import fec
    outs, fixed, failed = fec.ReedSolomonCodec(nsym, I).decode_batch(datas, erasures, return_status=True)
    assert len(outs) == len(fixed) == len(failed) == len(datas)
    return list(zip(outs, fixed, failed))


def gpu_encode(msgs, nsym, I=1):
    import fec
    return fec.ReedSolomonCodec(nsym, I).encode_batch(msgs)


_cache = {}


def corpus(nsym):
    """Per nsym, computed once: messages whose encodings end in every last-block
    length of LAST_BLOCKS (those the code has) over 1, 2 and 3 blocks, two of 20
    blocks, and the empty one; with the restatement's encodings."""
    if nsym not in _cache:
        rng = np.random.default_rng(700 + nsym)
        lasts = sorted({nsym + 1 if v is None else v for v in LAST_BLOCKS if v is None or v >= nsym + 1})
        lengths = [rc.msg_len_for_last_block(1 + i % 3, last, nsym) for i, last in enumerate(lasts)]
        lengths += [rc.msg_len_for_last_block(1 + (i + 1) % 3, last, nsym) for i, last in enumerate(lasts[:3])]
        short = len(lengths)
        lengths += [rc.msg_len_for_last_block(20, 255, nsym), rc.msg_len_for_last_block(20, nsym + 1, nsym), 0]
        msgs = rc.messages(rng, lengths)
        _cache[nsym] = (msgs, [rc.encode(m, nsym) for m in msgs], short)
    return _cache[nsym]


class Dev:
    """Device buffers for the *_device entries, freed on exit."""

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


def rows_of(datas, stride, pad):
    buf = np.full((len(datas), stride), pad, np.uint8)
    for i, r in enumerate(datas):
        buf[i, :len(r)] = np.frombuffer(r, np.uint8)
    return buf


def device_decode(rows, lens, in_stride, out_stride, nsym, I=1, mask=None, pad=0xA5, poison=0xEE):
    """amr_rs_decode_device on rows padded with `pad` to in_stride, every output
    pre-filled: (rc, out [n][out_stride], out_len, corrected, failed)."""
    n = len(rows)
    out = np.full((n, out_stride), poison, np.uint8)
    with Dev() as d:
        d_in, d_len = d.put(rows_of(rows, in_stride, pad)), d.put(np.asarray(lens, np.int64))
        d_er = d.put(mask) if mask is not None else None
        d_out, d_oln = d.put(out), d.put(np.full(n, -7, np.int64))
        d_cor, d_bad = d.put(np.full(n, -7, np.int32)), d.put(np.full(n, -7, np.int32))
        code = d.L.amr_rs_decode_device(None, d_in, in_stride, d_len, d_er, n, nsym, I, d_out, out_stride, d_oln,
                                        d_cor, d_bad)
        d.a.check(d.L.amr_device_synchronize())
        return (code, d.get(d_out, out), d.get(d_oln, np.zeros(n, np.int64)), d.get(d_cor, np.zeros(n, np.int32)),
                d.get(d_bad, np.zeros(n, np.int32)))


def device_encode(rows, lens, in_stride, out_stride, nsym, I=1, pad=0xA5, poison=0xEE):
    n = len(rows)
    out = np.full((n, out_stride), poison, np.uint8)
    with Dev() as d:
        d_in, d_len = d.put(rows_of(rows, in_stride, pad)), d.put(np.asarray(lens, np.int64))
        d_out, d_oln = d.put(out), d.put(np.full(n, -7, np.int64))
        code = d.L.amr_rs_encode_device(None, d_in, in_stride, d_len, n, nsym, I, d_out, out_stride, d_oln)
        d.a.check(d.L.amr_device_synchronize())
        return code, d.get(d_out, out), d.get(d_oln, np.zeros(n, np.int64))


# ---------------------------------------------------------------------------
def test_known_answers():
    import fec
    qr = bytes([32, 91, 11, 120, 209, 114, 220, 77, 67, 64, 236, 17, 236, 17, 236, 17])
    codec = fec.ReedSolomonCodec(10)
    assert codec.encode(qr) == qr + bytes([196, 35, 39, 119, 235, 215, 231, 226, 93, 23])
    assert codec.encode(b"hello world") == b"hello world" + bytes.fromhex("ed2554c4fdfd89f3a8aa")
    assert codec.encode(b"") == b"" and codec.encode_batch([]) == [] and codec.decode(b"") == b""
    rx = bytearray(codec.encode(b"hello world"))
    for p in (0, 5, 10, 13, 20):                            # five errors, parity bytes among them
        rx[p] ^= 0xFF
    assert codec.decode(bytes(rx)) == b"hello world"
    rx[7] ^= 1
    with pytest.raises(fec.ReedSolomonError):
        codec.decode(bytes(rx))
    assert codec.decode(bytes(rx), erase_pos=[0, 5]) == b"hello world"      # 2 * 4 + 2 <= 10


@pytest.mark.parametrize("nsym", NSYMS)
def test_encode_equals_the_restatement(nsym):
    msgs, cws, _ = corpus(nsym)
    assert gpu_encode(msgs, nsym) == cws                    # one ragged launch, 0 .. 20 blocks
    assert gpu_encode([msgs[0]], nsym) == [cws[0]]          # alone: a batch of one


@pytest.mark.parametrize("nsym", NSYMS)
def test_clean_and_corrupted_blocks_equal_the_restatement(nsym):
    """Clean input; exactly t, t - 1 and t + 1 errors in every block; errors in the
    parity bytes only; errors at the first and the last byte of every block."""
    msgs, cws, short = corpus(nsym)
    t = nsym // 2
    rng = np.random.default_rng(800 + nsym)
    rows, sent, kinds = list(cws), list(msgs), ["clean"] * len(cws)
    for kind, ne, where in (("t", t, "any"), ("t-1", t - 1, "any"), ("t+1", t + 1, "any"), ("parity", t, "parity"),
                            ("ends", max(t, 2), "ends")):
        pick = range(len(cws) - 1) if kind == "t" else range(short)      # the 20-block messages: clean and t only
        for i in pick:
            rows.append(rc.corrupt_blocks(rng, cws[i], nsym, 1, ne, where)[0])
            sent.append(msgs[i])
            kinds.append(kind)
    want = rc.decode_batch(rows, nsym)
    got = gpu_decode(rows, nsym)
    assert got == want
    for kind, msg, cw, (out, fixed, failed) in zip(kinds, sent, rows, got):
        nblk = len(rc.block_lens(len(cw)))
        if kind in ("clean", "t", "t-1", "parity") or (kind == "ends" and t >= 2):
            per = {"clean": 0, "t": t, "t-1": t - 1, "parity": min(t, nsym), "ends": t}[kind]
            assert (out, fixed, failed) == (msg, per * nblk, 0), kind
        else:                                               # beyond the code: a failure, or another codeword
            assert failed >= 1 or out != msg, kind
    assert any(f for _, _, f in got)


@pytest.mark.parametrize("nsym", NSYMS)
def test_erasures_equal_the_restatement(nsym):
    """Erasures alone up to nsym, mixed with errors up to the bound and one past
    it, more than nsym of them, and erased bytes that were right all along."""
    msgs, cws, short = corpus(nsym)
    rng = np.random.default_rng(900 + nsym)
    f_mix = nsym // 2
    e_mix = (nsym - f_mix) // 2
    plans = [("f=1", 0, 1, 0), ("f=nsym", 0, nsym, 1), ("mixed", e_mix, nsym - 2 * e_mix, 1),
             ("mixed+1", e_mix + 1, nsym - 2 * e_mix, 0), ("f=nsym+1", 0, nsym + 1, 0), ("right", 0, nsym, nsym)]
    rows, ers, sent, kinds = [], [], [], []
    for kind, ne, nf, right in plans:
        for i in range(0, short, 2):
            rx, er = rc.corrupt_blocks(rng, cws[i], nsym, 1, ne, n_erase=nf, erase_right=right)
            rows.append(rx)
            ers.append(er)
            sent.append(msgs[i])
            kinds.append(kind)
    ers[0] = np.array(ers[0], np.int32)                     # any integer sequence will do
    want = rc.decode_batch(rows, nsym, 1, ers)
    got = gpu_decode(rows, nsym, 1, ers)
    assert got == want
    for kind, msg, rx, (out, fixed, failed) in zip(kinds, sent, rows, got):
        if kind in ("mixed+1", "f=nsym+1"):
            assert failed >= 1 or out != msg, kind
        else:
            assert out == msg and failed == 0, kind
        if kind == "right":
            assert fixed == 0 and rx == rc.encode(msg, nsym)
    # the same rows without their erasure lists: another answer, the same agreement
    assert gpu_decode(rows[:8], nsym) == rc.decode_batch(rows[:8], nsym)
    assert gpu_decode(rows[:3], nsym, 1, [None, [], None]) == rc.decode_batch(rows[:3], nsym)


@pytest.mark.parametrize("batch", [1, 3, 4, 5, 257])
def test_batch_sizes_with_mixed_lengths(batch):
    """4 blocks per workgroup: batches below, at and past it; empty messages, clean
    rows, rows within and beyond the code and erasures, all in one launch."""
    nsym = 10
    rng = np.random.default_rng(1000 + batch)
    lengths = rng.integers(0, 600, batch)
    lengths[rng.integers(0, batch)] = 0
    msgs = rc.messages(rng, lengths)
    cws = gpu_encode(msgs, nsym)
    assert cws == [rc.encode(m, nsym) for m in msgs]
    rows, ers = [], []
    for cw in cws:
        rx, er = rc.corrupt_blocks(rng, cw, nsym, 1, int(rng.integers(0, 7)), n_erase=int(rng.integers(0, 4)))
        rows.append(rx)
        ers.append(er if rng.integers(0, 2) else None)
    assert gpu_decode(rows, nsym, 1, ers) == rc.decode_batch(rows, nsym, 1, ers)


@pytest.mark.parametrize("nsym,I", [(32, 1), (32, 2), (32, 5), (10, 64)])
def test_interleave_with_ragged_groups_and_bursts(nsym, I):
    t = nsym // 2
    rng = np.random.default_rng(1100 + I)
    shapes = [(1, nsym + 1), (I + 1, 100), (2 * I, 255), (2 * I + 1, 255)] + ([(3, 77), (I - 1, 200)] if I > 2 else [])
    msgs = rc.messages(rng, [rc.msg_len_for_last_block(nb, last, nsym) for nb, last in shapes])
    cws = [rc.encode(m, nsym, I) for m in msgs]
    assert gpu_encode(msgs, nsym, I) == cws
    rows, sent = list(cws), list(msgs)
    full = np.frombuffer(cws[2], np.uint8)                  # two full groups of I full blocks
    for start, extra in ((0, 0), (255 * I - I * t, 0), (255 * I + 11, 0), (40, 1), (255 * I + 11, 1)):
        rx = full.copy()
        rx[start:start + I * t + extra] ^= rng.integers(1, 256, I * t + extra, dtype=np.uint8)
        rows.append(rx.tobytes())
        sent.append(msgs[2])
    for i in (1, 3):                                        # bursts that end in the ragged last group
        rx = np.frombuffer(cws[i], np.uint8).copy()
        rx[-(t + 3):] ^= rng.integers(1, 256, t + 3, dtype=np.uint8)
        rows.append(rx.tobytes())
        sent.append(msgs[i])
    ers = [None] * len(rows)
    rx, er = rc.corrupt_blocks(rng, cws[1], nsym, I, 2, n_erase=nsym - 4, erase_right=2)
    rows.append(rx)
    ers.append(er)
    sent.append(msgs[1])
    want = rc.decode_batch(rows, nsym, I, ers)
    got = gpu_decode(rows, nsym, I, ers)
    assert got == want
    n = len(cws)
    assert [g[0] for g in got[:n + 3]] == sent[:n + 3] and all(g[2] == 0 for g in got[:n + 3])
    assert [g[1] for g in got[n:n + 3]] == [I * t] * 3      # a burst of I t bytes inside a group: t per block
    for g, m in zip(got[n + 3:n + 5], sent[n + 3:n + 5]):   # one byte longer: t + 1 in one block
        assert g[2] >= 1 or g[0] != m
    assert got[-1][0] == sent[-1] and got[-1][2] == 0


def test_device_entry_isolates_bad_lengths():
    """The device entry reads the lengths in HBM: a bad one costs only its own row;
    in_stride > L with the padding 0xA5, the output pre-poisoned, an erasure mask."""
    nsym, I = 16, 2
    in_stride, out_stride = 600, 600 - 3 * 16                # 600 = 2 * 255 + 90: the longest row has 3 blocks
    rng = np.random.default_rng(41)
    msgs = rc.messages(rng, [552, 100, 239, 240, 0, 300, 17, 478, 50])
    cws = [rc.encode(m, nsym, I) for m in msgs]
    assert max(len(c) for c in cws) == in_stride
    rows, mask = [], np.zeros((len(cws), in_stride), np.uint8)
    for i, cw in enumerate(cws):
        rx, er = rc.corrupt_blocks(rng, cw, nsym, I, 5, n_erase=6)
        rows.append(rx)
        mask[i, er] = 1 + i                                 # nonzero = erased
        mask[i, len(rx):] = 7                               # flags past a row's length belong to no block
    lens = [len(r) for r in rows]
    bad = {1: 16, 3: 256 + 15, 5: in_stride + 1, 7: -3}     # last block < nsym + 1 (twice), > in_stride, negative
    for i, v in bad.items():
        lens[i] = v
    code, out, oln, cor, fail = device_decode(rows, lens, in_stride, out_stride, nsym, I, mask)
    assert code == 0
    for i, rx in enumerate(rows):
        if i in bad:
            assert oln[i] == 0 and cor[i] == 0 and fail[i] == -1 and np.all(out[i] == 0xEE), i
            continue
        er = np.flatnonzero(mask[i, :lens[i]])
        dec, fixed, failed = rc.decode(rx, nsym, I, er)
        assert dec == msgs[i] or len(rx) == 0 or failed
        assert (oln[i], cor[i], fail[i]) == (len(dec), fixed, failed), i
        assert out[i, :oln[i]].tobytes() == dec and np.all(out[i, oln[i]:] == 0xEE), i   # nothing past out_len


def test_output_stride_at_and_below_the_need():
    """out_stride exactly what the longest row needs works; one byte less is an
    error before any device work, never an overrun."""
    nsym = 8
    rng = np.random.default_rng(42)
    msgs = rc.messages(rng, [494, 247, 1, 300])             # 494 = 2 * 247: in_stride 510 holds it exactly
    cws = [rc.encode(m, nsym) for m in msgs]
    lens = [len(c) for c in cws]
    code, out, oln, cor, fail = device_decode(cws, lens, 510, 494, nsym)
    assert code == 0 and oln.tolist() == [494, 247, 1, 300] and not cor.any() and not fail.any()
    assert all(out[i, :oln[i]].tobytes() == m for i, m in enumerate(msgs))
    assert np.all(out[1, 247:] == 0xEE) and np.all(out[2, 1:] == 0xEE)
    code, out, oln, cor, fail = device_decode(cws, lens, 510, 493, nsym)
    import _amr
    assert code == _amr.AMR_E_INVALID and b"out_stride" in _amr.lib().amr_last_error()
    assert np.all(out == 0xEE) and np.all(oln == -7) and np.all(cor == -7) and np.all(fail == -7)
    # a stride that ends inside a block's parity holds the full blocks only: 515 -> 510 -> 494
    code, out, oln, cor, fail = device_decode(cws, lens, 515, 494, nsym)
    assert code == 0 and oln.tolist() == [494, 247, 1, 300]
    # the encoder: 494 message bytes need 510; a row whose length exceeds in_stride is refused alone
    code, enc, eln = device_encode(msgs, [494, 247, 1, 300], 494, 510, nsym)
    assert code == 0 and eln.tolist() == lens and all(enc[i, :eln[i]].tobytes() == c for i, c in enumerate(cws))
    assert np.all(enc[1, eln[1]:] == 0xEE) and np.all(enc[2, eln[2]:] == 0xEE)
    code, enc, eln = device_encode(msgs, [494, 247, 1, 300], 494, 509, nsym)
    assert code == _amr.AMR_E_INVALID and np.all(enc == 0xEE) and np.all(eln == -7)
    code, enc, eln = device_encode(msgs, [494, 495, -1, 300], 494, 510, nsym)
    assert code == 0 and eln.tolist() == [510, -1, -1, lens[3]]
    assert np.all(enc[1] == 0xEE) and np.all(enc[2] == 0xEE) and enc[3, :eln[3]].tobytes() == cws[3]


def test_concatenated_with_the_convolutional_code():
    """messages -> RS(255,223) I = 2 -> K=7 convolutional -> 6 % of the coded bits
    inverted -> Viterbi -> RS.  The seed and the rate were picked on the CPU with
    the two restatements: the inner decoder alone leaves wrong bytes in every
    message, in bursts; the outer code leaves none."""
    import fec
    import viterbi_cases as vc
    msgs, outer, rx = rc.chain_case(seed=3, ber=0.06)
    rs, conv, vit = fec.ReedSolomonCodec(32, 2), fec.ConvolutionalEncoder(), fec.ViterbiDecoder()
    assert rs.encode_batch(msgs) == outer
    sent = conv.encode_batch(outer)
    assert sent == [vc.encode(o) for o in outer] and all(len(a) == len(b) for a, b in zip(sent, rx))
    inner = vit.decode_ml_batch(rx)
    assert inner == [d for d, _ in vc.decode_batch(rx)]
    wrong = [sum(a != b for a, b in zip(i, o)) for i, o in zip(inner, outer)]
    assert wrong == [26, 19, 6, 13]                         # the inner decoder alone does not recover them
    outs, fixed, failed = rs.decode_batch(inner, return_status=True)
    assert outs == msgs and fixed == wrong and failed == [0, 0, 0, 0]
    assert [rc.decode(i, 32, 2) for i in inner] == list(zip(outs, fixed, failed))
