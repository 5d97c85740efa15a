"""The Reed-Solomon code, host side (no GPU): the numpy restatement in
tests/rs_cases.py against known answers and against brute force -- every error
pattern within the bound, every codeword of the short codes with erasures --
and the C ABI's lengths and refusals."""
import numpy as np
import pytest

import rs_cases as rc

NEW_SYMBOLS = ["amr_rs_encoded_len", "amr_rs_decoded_len", "amr_rs_encode_host", "amr_rs_encode_device",
               "amr_rs_decode_host", "amr_rs_decode_device"]


@pytest.fixture(scope="module", autouse=True)
def product(built_lib):
    """The restatement is only worth testing beside the product it restates:
    every test here needs the library's new entries and fec's new class."""
    import _amr
    import fec
    L = _amr.lib()
    for name in NEW_SYMBOLS:
        assert name in _amr.EXPORTS and getattr(L, name).argtypes is not None, name
    for name in ("encode", "encode_batch", "decode", "decode_batch"):
        assert callable(getattr(fec.ReedSolomonCodec, name)), name
    assert issubclass(fec.ReedSolomonError, ValueError)
    return L


def u8(b):
    return np.frombuffer(bytes(b), np.uint8)


# ---- the field, the generator, known answers --------------------------------------
def test_field_tables():
    assert rc.EXP[0] == 1 and rc.EXP[1] == 2 and rc.EXP[8] == 0x1D and rc.EXP[254] == rc.inv(2)
    assert sorted(int(v) for v in rc.EXP[:255]) == list(range(1, 256))          # alpha = 2 is primitive
    rng = np.random.default_rng(0)
    for a, b, c in rng.integers(1, 256, (50, 3)):
        a, b, c = int(a), int(b), int(c)
        assert rc.mul(a, rc.inv(a)) == 1 and rc.mul(a, b) == rc.mul(b, a)
        assert rc.mul(a, b ^ c) == rc.mul(a, b) ^ rc.mul(a, c)
        slow = 0                                                                 # shift/xor, as the kernels multiply
        x = a
        for i in range(8):
            slow ^= x if (b >> i) & 1 else 0
            x = (x << 1) ^ (rc.POLY if x & 0x80 else 0)
        assert slow == rc.mul(a, b)


def test_generator_nsym_10():
    assert [int(rc.LOG[c]) for c in rc.generator(10)] == [0, 251, 67, 46, 61, 118, 70, 64, 94, 32, 45]
    for nsym in (2, 3, 32, 64):
        g = rc.generator(nsym)
        assert len(g) == nsym + 1 and g[0] == 1 and all(g)
        assert all(rc.poly_eval(g[::-1], int(rc.EXP[i])) == 0 for i in range(nsym))
        assert rc.poly_eval(g[::-1], int(rc.EXP[nsym])) != 0


def test_known_answers():
    qr = bytes([32, 91, 11, 120, 209, 114, 220, 77, 67, 64, 236, 17, 236, 17, 236, 17])
    assert rc.parity(u8(qr), 10).tolist() == [196, 35, 39, 119, 235, 215, 231, 226, 93, 23]
    assert rc.parity(u8(b"hello world"), 10).tobytes().hex() == "ed2554c4fdfd89f3a8aa"
    assert rc.encode(b"hello world", 10) == b"hello world" + bytes.fromhex("ed2554c4fdfd89f3a8aa")
    assert rc.encode(b"", 10) == b"" and rc.decode(b"", 10) == (b"", 0, 0)


def test_every_encoded_block_has_zero_syndromes():
    rng = np.random.default_rng(3)
    for nsym in (2, 3, 10, 32, 63, 64):
        k = 255 - nsym
        for n in (1, 2, k - 1, k, k + 1, 2 * k + 7):
            blocks = rc.encode_blocks(rc.messages(rng, [n])[0], nsym)
            assert [b.size for b in blocks] == rc.block_lens(rc.encoded_len(n, nsym))
            assert all(not rc.syndromes(b, nsym).any() for b in blocks), (nsym, n)


# ---- brute force --------------------------------------------------------------------
def _against_patterns(nsym, n, words, seed):
    """Random words, and codewords with 0 .. t + 2 errors: the decoder gives the
    pattern table's codeword exactly where there is one."""
    rng = np.random.default_rng(seed)
    table = rc.pattern_syndromes(n, nsym, nsym // 2)
    none = np.zeros(n, bool)
    found = failed = moved = 0
    for w in range(words):
        msg = rng.integers(0, 256, n - nsym, dtype=np.uint8)
        sent = np.concatenate([msg, rc.parity(msg, nsym)])
        if w % 2:
            rx = rng.integers(0, 256, n, dtype=np.uint8)
        else:
            rx = sent.copy()
            pos = rng.choice(n, min(n, w // 2 % (nsym // 2 + 3)), replace=False)
            rx[pos] ^= rng.integers(1, 256, pos.size, dtype=np.uint8)
        want = rc.brute_errors(rx, nsym, table)
        got, nfix = rc.decode_block(rx, none, nsym)
        if want is None:
            assert got is None, (nsym, n, rx.tobytes().hex())
            failed += 1
        else:
            assert got is not None and np.array_equal(got, want), (nsym, n, rx.tobytes().hex())
            assert nfix == np.count_nonzero(want != rx) <= nsym // 2
            found += 1
            moved += int(w % 2 == 0 and not np.array_equal(want, sent))
    return found, failed, moved


@pytest.mark.parametrize("n", range(3, 9))
def test_brute_force_nsym_2(n):
    found, failed, _ = _against_patterns(2, n, 300, seed=20 + n)
    assert found >= 50 and failed >= 50


def test_brute_force_nsym_2_miscorrects_beyond_capacity():
    moved = sum(_against_patterns(2, n, 300, seed=20 + n)[2] for n in (7, 8))
    assert moved >= 1                                       # two errors that land within one of ANOTHER codeword


@pytest.mark.parametrize("n", range(5, 9))
def test_brute_force_nsym_4(n):
    found, failed, _ = _against_patterns(4, n, 48, seed=40 + n)
    assert found >= 12 and failed >= 12


def test_pattern_table_agrees_with_the_codebook():
    """The pattern table itself, against the enumeration of every codeword."""
    rng = np.random.default_rng(7)
    for nsym, n in ((2, 4), (4, 6)):
        book = rc.codebook(n, nsym)
        assert book.shape == (65536, n) and all(not rc.syndromes(book[i], nsym).any() for i in (0, 1, 255, 256, 65535))
        table = rc.pattern_syndromes(n, nsym, nsym // 2)
        none = np.zeros(n, bool)
        for _ in range(40):
            rx = book[rng.integers(0, 65536)].copy()
            pos = rng.choice(n, rng.integers(0, n + 1), replace=False)
            rx[pos] ^= rng.integers(1, 256, pos.size, dtype=np.uint8)
            near = rc.brute_codebook(rx, none, nsym, book)
            want = rc.brute_errors(rx, nsym, table)
            assert len(near) == (want is not None) and (want is None or np.array_equal(near[0], want))


@pytest.mark.parametrize("nsym,n", [(2, 3), (2, 4), (4, 5), (4, 6)])
def test_brute_force_with_erasures(nsym, n):
    """f = 1 .. nsym + 1 erased positions, on random words and on codewords with
    errors: the decoder gives the one codeword within 2 e + f <= nsym, or fails."""
    rng = np.random.default_rng(100 * nsym + n)
    book = rc.codebook(n, nsym)
    found = failed = kept = 0
    for f in range(1, min(n, nsym + 1) + 1):
        for w in range(24):
            er = np.zeros(n, bool)
            er[rng.choice(n, f, replace=False)] = True
            if w % 3 == 0:
                rx = rng.integers(0, 256, n, dtype=np.uint8)
            else:
                rx = book[rng.integers(0, book.shape[0])].copy()
                ne = min(n - f, w % 3 - 1 + w % 2)
                pos = rng.choice(np.nonzero(~er)[0], ne, replace=False)
                rx[pos] ^= rng.integers(1, 256, ne, dtype=np.uint8)
                if w % 4:                                       # erased bytes usually hold noise; sometimes the right value
                    rx[er] = rng.integers(0, 256, f, dtype=np.uint8)
            near = rc.brute_codebook(rx, er, nsym, book)
            got, nfix = rc.decode_block(rx, er, nsym)
            assert len(near) <= 1                               # the distance makes it unique
            if f > nsym:
                assert len(near) == 0
            if len(near) == 0:
                assert got is None, (f, rx.tobytes().hex(), er)
                failed += 1
            else:
                assert got is not None and np.array_equal(got, near[0]), (f, rx.tobytes().hex(), er)
                assert nfix == np.count_nonzero(near[0] != rx)
                found += 1
                kept += int(np.count_nonzero((near[0] == rx) & er) > 0)
            noise = rx.copy()                                   # received values at erased positions are ignored
            noise[er] ^= 0x5A
            got2, _ = rc.decode_block(noise, er, nsym)
            assert (got2 is None) == (got is None) and (got is None or np.array_equal(got, got2))
    assert found >= 20 and failed >= 4 and kept >= 1


# ---- streams ------------------------------------------------------------------------
def test_closed_form_stream_position_equals_the_emitted_stream():
    for I in (1, 2, 5, 64):
        for nblk, last in ((1, 40), (2, 255), (3, 33), (5, 100), (6, 255), (7, 34), (11, 254), (64, 60), (66, 200)):
            lens = [255] * (nblk - 1) + [last]
            idx = rc.stream_index(lens, I)
            assert sorted(np.concatenate(idx).tolist()) == list(range(sum(lens)))
            for B in (0, 1, I - 1, I, nblk - 2, nblk - 1):
                if 0 <= B < nblk:
                    got = [rc.stream_pos(B, c, I, nblk, last) for c in range(lens[B])]
                    assert got == idx[B].tolist(), (I, nblk, last, B)


def test_interleave_round_trip_with_ragged_groups():
    rng = np.random.default_rng(9)
    nsym = 32
    for I, nblk, last in ((2, 3, 40), (5, 7, 255), (5, 11, 33), (64, 3, 100), (4, 4, 77), (3, 1, 50)):
        msg = rc.messages(rng, [rc.msg_len_for_last_block(nblk, last, nsym)])[0]
        cw = rc.encode(msg, nsym, I)
        assert len(cw) == rc.encoded_len(len(msg), nsym) == 255 * (nblk - 1) + last
        assert rc.decode(cw, nsym, I) == (msg, 0, 0)
        if I > 1 and nblk > 1:
            assert cw != rc.encode(msg, nsym, 1) and sorted(cw) == sorted(rc.encode(msg, nsym, 1))
        plain = b"".join(b.tobytes() for b in rc.encode_blocks(msg, nsym))
        assert rc.encode(msg, nsym, 1) == plain and plain[:min(223, len(msg))] == msg[:223]   # I = 1: the concatenation


def test_burst_of_I_times_t_decodes_and_one_more_does_not():
    rng = np.random.default_rng(10)
    longer_fails = 0
    for nsym, I in ((32, 4), (10, 5), (3, 2), (64, 2)):
        t = nsym // 2
        msg = rc.messages(rng, [rc.msg_len_for_last_block(2 * I, 255, nsym)])[0]       # two full groups
        cw = u8(rc.encode(msg, nsym, I))
        for start in (0, 17, 255 * I - I * t, 255 * I + 3):
            rx = cw.copy()
            rx[start:start + I * t] ^= rng.integers(1, 256, I * t, dtype=np.uint8)
            if start + I * t <= 255 * I or start >= 255 * I:       # inside one group: t bytes per block at most
                out, fixed, failed = rc.decode(rx.tobytes(), nsym, I)
                assert (out, fixed, failed) == (msg, I * t, 0), (nsym, I, start)
            rx = cw.copy()
            rx[start:start + I * t + 1] ^= rng.integers(1, 256, I * t + 1, dtype=np.uint8)
            if start + I * t + 1 <= 255 * I or start >= 255 * I:   # t + 1 in one block of the group
                out, fixed, failed = rc.decode(rx.tobytes(), nsym, I)
                assert failed >= 1 or out != msg, (nsym, I, start)   # 2 (t + 1) > nsym: a failure or another codeword
                longer_fails += 1
    assert longer_fails >= 4


def test_restated_decode_counts():
    rng = np.random.default_rng(12)
    msg = rc.messages(rng, [500])[0]
    cw = rc.encode(msg, 32)
    rx, er = rc.corrupt_blocks(rng, cw, 32, 1, n_err=5, n_erase=20, erase_right=20)
    assert rc.decode(rx, 32, 1, er) == (msg, 15, 0)              # erased bytes that were right count 0
    rx, er = rc.corrupt_blocks(rng, cw, 32, 1, n_err=17)
    out, fixed, failed = rc.decode(rx, 32)
    assert failed == 3 and fixed == 0 and out == b"".join(bytes(u8(rx)[i:i + 255][:-32]) for i in (0, 255, 510))


# ---- the ABI: lengths and refusals ------------------------------------------------
def test_length_functions(product):
    L = product
    for nsym in (2, 10, 32, 64):
        k = 255 - nsym
        for n in (0, 1, k - 1, k, k + 1, 20 * k, 20 * k + 1):
            enc = L.amr_rs_encoded_len(n, nsym)
            assert enc == rc.encoded_len(n, nsym) == n + -(-n // k) * nsym
            assert L.amr_rs_decoded_len(enc, nsym) == n
    assert L.amr_rs_encoded_len(4460, 32) == 5100
    assert L.amr_rs_encoded_len(-1, 32) < 0 and L.amr_rs_encoded_len(5, 1) < 0 and L.amr_rs_encoded_len(5, 65) < 0


def test_invalid_length_table(product):
    import _amr
    import fec
    L = product
    table = {2: {0: 0, 1: -1, 2: -1, 3: 1, 255: 253, 256: -1, 257: -1, 258: 254, 510: 506},
             32: {0: 0, 1: -1, 32: -1, 33: 1, 254: 222, 255: 223, 256: -1, 287: -1, 288: 224, 5100: 4460, 5101: -1},
             64: {64: -1, 65: 1, 255: 191, 319: -1, 320: 192}}
    for nsym, rows in table.items():
        for n, want in rows.items():
            assert L.amr_rs_decoded_len(n, nsym) == want, (nsym, n)
            assert rc.decoded_len(n, nsym) == want and _amr.rs_decoded_len(n, nsym) == want
            assert fec.ReedSolomonCodec(nsym).decoded_len(n) == want
    assert L.amr_rs_decoded_len(-1, 32) == -1 and L.amr_rs_decoded_len(33, 1) < 0 and L.amr_rs_decoded_len(66, 65) < 0


def test_decode_device_refusals(product):
    """Bad arguments are refused, with a message, before any device work."""
    import _amr
    L = product
    buf = np.zeros((2, 300), np.uint8)
    out = np.zeros((2, 268), np.uint8)
    ln = np.array([300, 300], np.int64)
    oln = np.zeros(2, np.int64)
    cor = np.zeros(2, np.int32)
    bad = np.zeros(2, np.int32)
    p = _amr.ptr

    def call(d_in=p(buf), in_stride=300, d_len=p(ln), d_er=None, n=2, nsym=16, il=1, d_out=p(out), out_stride=268,
             d_oln=p(oln), d_cor=p(cor), d_bad=p(bad)):
        return L.amr_rs_decode_device(None, d_in, in_stride, d_len, d_er, n, nsym, il, d_out, out_stride, d_oln,
                                      d_cor, d_bad)

    for kw, word in (({"n": -1}, b"negative"), ({"in_stride": -1}, b"negative"), ({"out_stride": -1}, b"negative"),
                     ({"nsym": 1}, b"nsym"), ({"nsym": 65}, b"nsym"), ({"il": 0}, b"interleave"),
                     ({"il": 65}, b"interleave"), ({"d_in": None}, b"NULL"), ({"d_len": None}, b"NULL"),
                     ({"d_out": None}, b"NULL"), ({"d_oln": None}, b"NULL"), ({"d_cor": None}, b"NULL"),
                     ({"d_bad": None}, b"NULL"), ({"out_stride": 267}, b"out_stride")):   # 300 = 255 + 45: 239 + 29 = 268
        assert call(**kw) == _amr.AMR_E_INVALID, kw
        assert word in L.amr_last_error(), (kw, L.amr_last_error())
    # a stride whose last block cannot be valid holds the full blocks only: 270 = 255 + 15 gives 239
    assert call(in_stride=270, out_stride=238) == _amr.AMR_E_INVALID
    assert call(n=0, d_in=None, d_len=None, d_out=None, d_oln=None, d_cor=None, d_bad=None) == _amr.AMR_OK
    assert not out.any() and not oln.any() and not cor.any() and not bad.any()


def test_encode_device_refusals(product):
    import _amr
    L = product
    buf = np.zeros((2, 300), np.uint8)
    out = np.zeros((2, 332), np.uint8)
    ln = np.array([300, 300], np.int64)
    oln = np.zeros(2, np.int64)
    p = _amr.ptr

    def call(d_in=p(buf), in_stride=300, d_len=p(ln), n=2, nsym=16, il=1, d_out=p(out), out_stride=332, d_oln=p(oln)):
        return L.amr_rs_encode_device(None, d_in, in_stride, d_len, n, nsym, il, d_out, out_stride, d_oln)

    for kw, word in (({"n": -1}, b"negative"), ({"in_stride": -1}, b"negative"), ({"out_stride": -1}, b"negative"),
                     ({"nsym": 1}, b"nsym"), ({"nsym": 65}, b"nsym"), ({"il": 0}, b"interleave"),
                     ({"il": 65}, b"interleave"), ({"d_in": None}, b"NULL"), ({"d_len": None}, b"NULL"),
                     ({"d_out": None}, b"NULL"), ({"d_oln": None}, b"NULL"),
                     ({"out_stride": 331}, b"out_stride")):                               # 300 + 2 * 16
        assert call(**kw) == _amr.AMR_E_INVALID, kw
        assert word in L.amr_last_error(), (kw, L.amr_last_error())
    assert call(n=0, d_in=None, d_len=None, d_out=None, d_oln=None) == _amr.AMR_OK
    assert not out.any() and not oln.any()


def test_host_entry_refusals(product):
    import _amr
    L = product
    buf = np.zeros((3, 300), np.uint8)
    out = np.zeros((3, 332), np.uint8)
    oln = np.zeros(3, np.int64)
    cor = np.zeros(3, np.int32)
    bad = np.zeros(3, np.int32)
    p = _amr.ptr

    def dec(lens, in_=p(buf), in_stride=300, er=None, n=3, nsym=16, il=1, out_=p(out), out_stride=268, oln_=p(oln),
            cor_=p(cor), bad_=p(bad)):
        ln = np.array(lens, np.int64)
        return L.amr_rs_decode_host(in_, in_stride, p(ln), er, n, nsym, il, out_, out_stride, oln_, cor_, bad_)

    for v in (1, 16, 256, 271, 301, -2):                    # last block below nsym + 1, > in_stride, negative
        assert dec([300, 17, v]) == _amr.AMR_E_INVALID, v
        msg = L.amr_last_error()
        assert b"row 2" in msg and str(v).encode() in msg, msg
    assert dec([300, 5, 300]) == _amr.AMR_E_INVALID and b"row 1" in L.amr_last_error()
    for kw in ({"n": -1}, {"in_stride": -1}, {"out_stride": -1}, {"nsym": 1}, {"nsym": 65}, {"il": 0}, {"il": 65},
               {"in_": None}, {"out_": None}, {"oln_": None}, {"cor_": None}, {"bad_": None}, {"out_stride": 267}):
        assert dec([300, 300, 300], **kw) == _amr.AMR_E_INVALID, kw
    assert L.amr_rs_decode_host(p(buf), 300, None, None, 3, 16, 1, p(out), 268, p(oln), p(cor), p(bad)) \
        == _amr.AMR_E_INVALID
    assert L.amr_rs_decode_host(None, 0, None, None, 0, 16, 1, None, 0, None, None, None) == _amr.AMR_OK

    def enc(lens, in_=p(buf), in_stride=300, n=3, nsym=16, il=1, out_=p(out), out_stride=332, oln_=p(oln)):
        ln = np.array(lens, np.int64)
        return L.amr_rs_encode_host(in_, in_stride, p(ln), n, nsym, il, out_, out_stride, oln_)

    assert enc([300, 301, 0]) == _amr.AMR_E_INVALID and b"row 1" in L.amr_last_error()
    assert enc([-1, 300, 0]) == _amr.AMR_E_INVALID and b"row 0" in L.amr_last_error()
    for kw in ({"n": -1}, {"in_stride": -1}, {"out_stride": -1}, {"nsym": 1}, {"nsym": 65}, {"il": 0}, {"il": 65},
               {"in_": None}, {"out_": None}, {"oln_": None}, {"out_stride": 331}):
        assert enc([300, 300, 300], **kw) == _amr.AMR_E_INVALID, kw
    assert L.amr_rs_encode_host(p(buf), 300, None, 3, 16, 1, p(out), 332, p(oln)) == _amr.AMR_E_INVALID
    assert L.amr_rs_encode_host(None, 0, None, 0, 16, 1, None, 0, None) == _amr.AMR_OK
    assert not out.any() and not oln.any() and not cor.any() and not bad.any()


def test_python_argument_errors_come_before_any_device_work(product):
    import fec
    for kw in ({"nsym": 1}, {"nsym": 65}, {"interleave": 0}, {"interleave": 65}):
        with pytest.raises(ValueError):
            fec.ReedSolomonCodec(**kw)
    codec = fec.ReedSolomonCodec()
    assert (codec.nsym, codec.interleave) == (32, 1)
    for n in (1, 32, 256, 287):
        with pytest.raises(fec.ReedSolomonError):
            codec.decode(bytes(n))
    with pytest.raises(ValueError) as e:
        codec.decode_batch([bytes(33), bytes(40), bytes(256)], return_status=True)
    assert "row 2" in str(e.value) and not isinstance(e.value, fec.ReedSolomonError)
    stub = fec.ReedSolomonFEC()                              # the parity class is still the reference's
    assert stub.encode(b"abc") == b"ab\x03c\xff" + (0x352441C2).to_bytes(4, "little")


def test_no_gpu_is_an_error_not_a_fallback(product):
    import _amr
    import fec
    if _amr.device_count() > 0:
        return                                              # the GPU suite covers the working path
    codec = fec.ReedSolomonCodec(10, 2)
    with pytest.raises(_amr.AmrError):
        codec.encode(b"abc")
    with pytest.raises(_amr.AmrError):
        codec.encode_batch([b"abc", b""])
    with pytest.raises(_amr.AmrError):
        codec.decode(bytes(40), erase_pos=[1, 2])
    with pytest.raises(_amr.AmrError):
        codec.decode_batch([bytes(40), bytes(11)], return_status=True)
    with pytest.raises(_amr.AmrError):
        _amr.rs_encode([b"x"], 32, 1)
    with pytest.raises(_amr.AmrError):
        _amr.rs_decode([bytes(40)], 32, 1, None)
