"""Hellschreiber on the GPU (hell_kernels.hip, AMR_TX_HELL in tx_kernels.hip)
against the reference's recorded outputs (tests/golden/hell.npz), np.mean(chunk ** 2)
itself, and the restatement in tests/hell_cases.py.

Receiver: bytes and per-pixel energies are bit-exact.  Modulator: the bound of
tests/test_gpu_tx.py, argued there for exactly this situation -- sin() is the
only inexact operation (ocml on the GPU, libm on the host, both within 1 ulp
in float64), which reaches the float32 sample only when the double lands within
~1 ulp64 of a float32 rounding boundary: at most 1 ulp (float32) per sample, on
at most 1e-6 of the samples (+1), the int16 WAV samples within 1 where the
float32 differs and equal elsewhere."""
import ctypes
import json
import os

import numpy as np
import pytest

import hell_cases as hc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")

# sps -> (baud, samp_rate) that give it through int(round(samp_rate / baud))
SPS_PARAMS = {5: (19200, 96000), 9: (10666, 96000), 128: (750, 96000), 129: (744.2, 96000), 136: (705.9, 96000),
              784: (122.5, 96000), 8192: (1, 8192), 8193: (1, 8193), 19200: (5, 96000)}
ELEMS = ["float32", "float64", "float16", "int16", "uint8", "int32", "pcm16"]


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")


@pytest.fixture(scope="module")
def hell():
    with open(os.path.join(G, "hell_manifest.json")) as f:
        return json.load(f)["cases"], np.load(os.path.join(G, "hell.npz"))


@pytest.fixture(scope="module")
def lut():
    return hc.lookup_table()


def ulps(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    def ordered(x):
        i = x.astype(np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def assert_close(got, want, pcm_got=None, pcm_want=None, what=""):
    assert got.shape == want.shape and got.dtype == np.float32, what
    u = ulps(got, want)
    bad = np.count_nonzero(u)
    assert u.max(initial=0) <= 1, f"{what}: {u.max()} ulp"
    assert bad <= 1 + got.size * 1e-6, f"{what}: {bad} of {got.size} samples differ"
    if pcm_got is not None:
        dp = np.abs(pcm_got.astype(np.int32) - pcm_want.astype(np.int32))
        assert dp.max(initial=0) <= 1 and np.all(dp[u == 0] == 0), what
    return bad


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and np.array_equal(a.astype(np.float64).view(np.uint64), b.astype(np.float64).view(np.uint64))


def bytes_from_bits(bits: np.ndarray, lut: bytes) -> bytes:
    n = bits.size // 7
    v = (bits[:7 * n].reshape(n, 7).astype(np.int64) << np.arange(7)).sum(axis=1)
    return bytes(lut[int(k)] for k in v)


# ---------------------------------------------------------------------------
# demodulator bytes against the reference's recorded outputs
def test_demodulator_bytes_equal_reference_fixtures(hell):
    import modem
    cases, d = hell
    n = 0
    for c in cases:
        if c["kind"] != "rx":
            continue
        x = d[c["id"] + ".in"]
        p = c["params"]
        baud, carrier, sr = p.get("baud", 122.5), p.get("carrier", 1000.0), p.get("samp_rate", 96000)
        if c["status"] == "err":
            with pytest.raises(ValueError) as e:
                modem.feld_hell_demodulate(x, baud, carrier, sr)
            assert str(e.value) == c["emsg"], c["id"]
            with pytest.raises(ValueError) as e:
                modem.feld_hell_demodulate_batch(x[None, :], baud, carrier, sr)
            assert str(e.value) == c["emsg"], c["id"]
            continue
        want = bytes.fromhex(c["out"])
        assert modem.feld_hell_demodulate(x, baud, carrier, sr) == want, c["id"]
        got = modem.feld_hell_demodulate_batch(np.stack([x, x, x]), baud, carrier, sr)
        assert got == [want] * 3, c["id"]
        n += 1
    assert n >= 20


def test_pcm16_form_equals_float64_of_the_same_wav(lut):
    """decoder._Pcm16's internal form: int16 PCM converted on the device ==
    the reference on pcm / 32768.0 (float64)."""
    import modem
    rng = np.random.default_rng(16)
    pcm = (rng.normal(0, 0.316, 7 * 11 * 784 + 50) * 32768).clip(-32768, 32767).astype(np.int16)
    want = hc.demodulate(pcm / 32768.0, 122.5, 96000, lut)
    assert len(want) == 11 and modem._pcm16_hell(pcm) == want
    assert modem.feld_hell_demodulate(pcm / 32768.0, 122.5, 1000.0) == want


# ---------------------------------------------------------------------------
# energies, bit for bit against np.mean(chunk ** 2)
def draw(rng, elem, shape):
    if elem in ("float32", "float64", "float16"):
        return rng.normal(0.0, 0.33, shape).astype(elem)        # mean square ~0.11: decisions on both sides
    if elem in ("int16", "pcm16"):
        return rng.integers(-32768, 32768, shape).astype(np.int16)   # full scale: raw int16 squares wrap
    if elem == "uint8":
        return rng.integers(0, 256, shape).astype(np.uint8)
    return rng.integers(-2**31, 2**31, shape).astype(np.int32)


def numpy_energy_rows(x, sps, elem):
    """np.mean(chunk ** 2) per pixel and row, exactly as the reference calls it; float64-widened."""
    rows = []
    for r in x:
        rr = r / 32768.0 if elem == "pcm16" else r
        rows.append(hc.numpy_energies(rr, sps).astype(np.float64))
    return np.stack(rows)


def decisions(x, sps, elem):
    out = []
    for r in x:
        rr = r / 32768.0 if elem == "pcm16" else r
        with np.errstate(all="ignore"):
            out.append(np.array([np.mean(rr[i:i + sps] ** 2) > 0.1 for i in range(0, rr.size - sps + 1, sps)], bool))
    return np.stack(out)


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("sps", sorted(SPS_PARAMS))
def test_energies_equal_numpy_mean(sps, elem, lut):
    import _amr
    baud, sr = SPS_PARAMS[sps]
    assert hc.sps_of(baud, sr) == sps
    code = _amr.HELL_PCM16 if elem == "pcm16" else None
    rng = np.random.default_rng(7919 * sps + ELEMS.index(elem))
    n_max = 23 * sps + 5
    X = draw(rng, elem, (3, n_max + 9))                          # every call below: row stride > N
    ref = numpy_energy_rows(X[:, :n_max], sps, elem)             # [3][23], computed once
    dec = decisions(X[:, :n_max], sps, elem)
    for n in (sps - 1, sps, 7 * sps - 1, 7 * sps, 7 * sps + 3, n_max):
        n_pix = n // sps
        for B in (3, 1):
            outs, en = _amr.hell_demod(X[:B, :n], baud, sr, elem=code, energy=True)
            assert en.shape == (B, n_pix)
            assert same_bits(en, ref[:B, :n_pix]), (sps, elem, n, B)
            assert outs == [bytes_from_bits(dec[b, :n_pix], lut) for b in range(B)], (sps, elem, n, B)
    # rows that start one element into the buffer: odd offsets for every pixel start
    n = 7 * sps + 3
    Y = X[:, 1:n + 1]
    outs, en = _amr.hell_demod(Y, baud, sr, elem=code, energy=True)
    assert same_bits(en, numpy_energy_rows(Y, sps, elem)), (sps, elem, "offset 1")
    # 257 streams (more than one block of waves per pixel group), rows 0..2 repeated
    idx = np.arange(257) % 3
    big = np.ascontiguousarray(X[idx, :n])
    outs, en = _amr.hell_demod(big, baud, sr, elem=code, energy=True)
    assert same_bits(en, ref[idx, :7]), (sps, elem, 257)
    assert outs == [bytes_from_bits(dec[b, :7], lut) for b in idx]
    assert _amr.hell_demod(big, baud, sr, elem=code) == outs      # without the energy buffer: the same bytes


def test_integer_widths_and_bool(lut):
    """Every integer width and signedness squares in its own dtype; bool ** 2 is int8."""
    import modem
    rng = np.random.default_rng(99)
    for dt in (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64):
        info = np.iinfo(dt)
        x = rng.integers(info.min, info.max, 7 * 9 * 9 + 4, dtype=dt, endpoint=True)
        x[::3] = rng.integers(0, 2, x[::3].size).astype(dt)     # some small pixels too
        assert modem.feld_hell_demodulate(x, 10666, 1000.0) == hc.demodulate(x, 10666, 96000, lut), dt
    b = rng.random(7 * 30 * 9) < 0.1
    want = bytes_from_bits(decisions(b[None, :], 9, "bool")[0], lut)
    assert modem.feld_hell_demodulate(b, 10666, 1000.0) == want
    with pytest.raises(TypeError):
        modem.feld_hell_demodulate(np.zeros(100, np.complex128), 10666, 1000.0)


# ---------------------------------------------------------------------------
# the threshold's edge
@pytest.mark.parametrize("dtype", ["float32", "float64", "float16"])
def test_threshold_edge(dtype, lut):
    """Pixels whose energy lands within a few ulps of the threshold, both sides,
    and pixels whose energy IS float32(0.1) / float16(0.1) / 0.1: numpy's `>`."""
    import _amr
    dt = np.dtype(dtype)
    rng = np.random.default_rng(31)
    # (a) sps 784: each pixel scaled so that its energy rounds to about the threshold
    sps, n_pix = 784, 7 * 40
    px = rng.normal(0.0, 0.3, (n_pix, sps))
    px *= np.sqrt(0.1 / np.mean(px.astype(dt).astype(np.float64) ** 2, axis=1))[:, None]
    x = px.astype(dt).ravel()
    ref = hc.numpy_energies(x, sps)
    thr = hc.threshold(dt)
    bits = ref > thr
    assert bits.any() and not bits.all()
    assert np.abs(ref.astype(np.float64) - float(thr)).max() <= 8 * float(np.spacing(thr))
    outs, en = _amr.hell_demod(x[None, :], 122.5, 96000, energy=True)
    assert same_bits(en[0], ref)
    assert outs[0] == bytes_from_bits(bits, lut)
    # (b) sps 5: [0.5, 0.5, 0, 0, 0] has energy 0.5 / 5, which rounds to exactly the dtype's 0.1
    exact = np.array([0.5, 0.5, 0, 0, 0], dt)
    up = exact.copy()
    up[1] = np.nextafter(dt.type(0.5), dt.type(1))
    down = exact.copy()
    down[1] = np.nextafter(dt.type(0.5), dt.type(0))
    chunks = [exact, up, down, exact, up, exact, down] * 6
    y = np.concatenate(chunks)
    ref = hc.numpy_energies(y, 5)
    assert np.count_nonzero(ref == thr) >= 18
    bits = ref > thr
    assert not bits[0]                                   # equal to the threshold is not above it
    outs, en = _amr.hell_demod(y[None, :], 19200, 96000, energy=True)
    assert same_bits(en[0], ref)
    assert outs[0] == bytes_from_bits(bits, lut)


# ---------------------------------------------------------------------------
# modulator
def expected_wave(d, cid):
    bits, row, pcmrow = d[cid + ".bits"], d[cid + ".row"], d[cid + ".pcmrow"]
    return (bits[:, None] * row[None, :]).ravel().astype(np.float32), (bits[:, None] * pcmrow[None, :]).ravel().astype(np.int16)


def test_modulator_matches_reference_fixtures(hell):
    import modem
    cases, d = hell
    seen = set()
    for c in cases:
        if c["kind"] != "tx":
            continue
        p = c["params"]
        if c["fn"] == "feld_hell_modulate":
            call = lambda: modem.feld_hell_modulate(bytes.fromhex(c["data"]), p["baud"], p["carrier"], p["samp_rate"])  # noqa: E731
        else:
            call = lambda: modem.hellschreiber_modulate(c["text"], **p)  # noqa: E731
        if c["status"] == "err":
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == c["emsg"], c["id"]
            continue
        y = call()
        want, pcm_want = expected_wave(d, c["id"])
        assert want.size == c["n"]
        wav = modem.wav_from_array(y)
        assert wav[:44].hex() == c["wav_header"], c["id"]
        assert_close(y, want, np.frombuffer(wav[44:], np.int16), pcm_want, what=c["id"])
        seen.add(c["id"])
    assert {"tx_default", "tx_outofmap", "tx_empty", "tx_carrier0", "tx_baud5"} <= seen
    assert not d["tx_carrier0.bits"].any()               # carrier 0: all zeros, the normalisation skipped


def pixel_bits(text: str, glyphs: dict) -> np.ndarray:
    px = [1] * 70
    for ch in text:
        px += (glyphs[ch] + [0, 0]) if ch in glyphs else [0] * 51
    return np.array(px + [1] * 35, np.uint8)


def test_batch_cut_pad_and_pcm(hell):
    """modulate_batch("hell"): rows == the single-text waveforms cut / zero-padded to
    n_out, and the int16 PCM == wav_from_array's samples.  Expected waveforms:
    the recorded glyph pixels x the reference's recorded on-pixel row for these parameters."""
    import modem
    cases, d = hell
    fast = next(c for c in cases if c["id"] == "tx_fast")
    baud, carrier = fast["params"]["baud"], fast["params"]["carrier"]
    row, pcmrow = d["tx_fast.row"], d["tx_fast.pcmrow"]
    glyphs = hc.glyph_pixels()
    texts = ["The quick brown fox", "", "A\tz~", b"ok \xff\xc3\xa9"]
    full = []
    for t in texts:
        s = t if isinstance(t, str) else t.decode("utf-8", "ignore")
        full.append(pixel_bits(s, glyphs))
    assert np.array_equal(full[0], d["tx_fast.bits"])
    n_out = full[0].size * row.size - 37                  # cuts the longest mid-pixel, pads the rest
    out, pcm = modem.modulate_batch("hell", texts, baud=baud, f0=carrier, n_out=n_out, pcm=True)
    assert out.shape == (4, n_out) and pcm.shape == (4, n_out) and pcm.dtype == np.int16
    for i, bits in enumerate(full):
        w = (bits[:, None] * row[None, :]).ravel()[:n_out]
        q = (bits[:, None] * pcmrow[None, :]).ravel()[:n_out]
        want = np.zeros(n_out, np.float32)
        want[:w.size] = w
        pw = np.zeros(n_out, np.int16)
        pw[:q.size] = q
        assert_close(out[i], want, pcm[i], pw, what=f"hell[{i}]")
    natural = modem.modulate_batch("hell", texts[:2], baud=baud, f0=carrier)
    assert natural.shape == (2, full[0].size * row.size) and not natural[1, full[1].size * row.size:].any()


# ---------------------------------------------------------------------------
def test_loopback_batch_of_64(lut):
    """Modulate, add seeded noise, demodulate 64 streams at once: the bytes are
    the restatement's on the same float32 samples."""
    import modem
    wave = modem.hellschreiber_modulate("HI 5")
    rng = np.random.default_rng(64)
    x = (wave[None, :] + rng.normal(0.0, 0.31, (64, wave.size))).astype(np.float32)   # off-pixels near the threshold
    got = modem.feld_hell_demodulate_batch(x)
    want = [hc.demodulate(r, 122.5, 96000, lut) for r in x]
    assert got == want and len(set(got)) > 1 and len(got[0]) == (105 + 51 * 4) // 7
    assert modem.feld_hell_demodulate(x[5], 122.5, 1000.0) == want[5]


def test_device_entry_on_a_plan_stream():
    """amr_hell_demod_device enqueued on a plan's stream == the host entry."""
    import _amr
    L = _amr.lib()
    rng = np.random.default_rng(12)
    B, n, stride = 5, 23 * 784 + 5, 23 * 784 + 64
    x = np.zeros((B, stride), np.float32)
    x[:, :n] = rng.normal(0.0, 0.33, (B, n))
    want, want_en = _amr.hell_demod(x[:, :n], 122.5, 96000, energy=True)
    plan = _amr.get_psk_plan("qpsk", 24000, 9600, 3000.0, 96000, 1)
    n_pix = int(L.amr_hell_pixels(n, 122.5, 96000.0))
    wb = int(L.amr_hell_work_bytes(122.5, 96000.0))
    assert n_pix == 23 and wb > 0
    sizes = [x.nbytes, B * 8, B * 8, B * n_pix * 8, wb]
    bufs = []
    try:
        for sz in sizes:
            p = ctypes.c_void_p()
            _amr.check(L.amr_malloc(ctypes.byref(p), sz))
            bufs.append(p)
        d_x, d_out, d_len, d_en, d_work = bufs
        _amr.check(L.amr_memcpy_h2d(d_x, _amr.ptr(x), x.nbytes))
        _amr.check(L.amr_hell_demod_device(plan.handle, d_x, 0, B, stride, n, 122.5, 96000.0, d_out, 8, d_len, d_en,
                                           d_work, wb))
        _amr.check(L.amr_psk_plan_synchronize(plan.handle))
        out = np.zeros((B, 8), np.uint8)
        ln = np.zeros(B, np.int64)
        en = np.zeros((B, n_pix))
        _amr.check(L.amr_memcpy_d2h(_amr.ptr(out), d_out, out.nbytes))
        _amr.check(L.amr_memcpy_d2h(_amr.ptr(ln), d_len, ln.nbytes))
        _amr.check(L.amr_memcpy_d2h(_amr.ptr(en), d_en, en.nbytes))
    finally:
        for p in bufs:
            L.amr_free(p)
    assert ln.tolist() == [3] * B
    assert [out[i, :3].tobytes() for i in range(B)] == want and same_bits(en, want_en)
    # NULL buffers are refused before any device work
    assert L.amr_hell_demod_device(None, None, 0, 1, 10, 10, 122.5, 96000.0, None, 0, None, None, None, 0) == _amr.AMR_E_INVALID


def test_abi_additions():
    import _amr
    L = _amr.lib()
    assert L.amr_abi_version() == 5
    for name in ("amr_hell_pixels", "amr_hell_work_bytes", "amr_hell_demod_host", "amr_hell_demod_device",
                 "amr_hell_glyph_rows"):
        assert getattr(L, name) is not None
    assert _amr.TX_MODES["hell"] == _amr.TX_HELL == 3
    assert L.amr_tx_samples(_amr.TX_HELL, 4, 122.5, 96000.0) == (105 + 51 * 4) * 784
    assert L.amr_tx_work_bytes(_amr.TX_HELL, 5.0, 96000.0, 2, 1000) > 19200 * 4
    assert L.amr_hell_pixels(96000, 122.5, 96000.0) == 122
    assert L.amr_hell_pixels(96000, 200000.0, 96000.0) == _amr.AMR_E_INVALID
    assert L.amr_last_error() == b"range() arg 3 must not be zero"
