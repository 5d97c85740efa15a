"""Hellschreiber receiver, host side (no GPU): the restatement in
tests/hell_cases.py against the reference's recorded outputs and against
np.mean(chunk ** 2) itself, the glyph bitmaps the product carries against the
recorded pixels, and the reference's error contract."""
import json
import os

import numpy as np
import pytest

import hell_cases as hc

G = os.path.join(os.path.dirname(__file__), "golden")
SPS = [5, 9, 128, 129, 136, 784, 8192, 8193, 19200]
DTYPES = ["float32", "float64", "float16", "int16", "uint8"]


@pytest.fixture(scope="module")
def hell():
    with open(os.path.join(G, "hell_manifest.json")) as f:
        return json.load(f)["cases"], np.load(os.path.join(G, "hell.npz"))


def draw(rng, dtype, n):
    """Samples whose pixel energies straddle nothing in particular: the sum order is the subject."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return rng.normal(0.0, 0.4, n).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max + 1, n).astype(dtype)      # full scale: int16 squares wrap


def test_restatement_equals_recorded_reference_outputs(hell):
    cases, d = hell
    n = 0
    for c in cases:
        if c["kind"] != "rx":
            continue
        x = d[c["id"] + ".in"]
        assert str(x.dtype) == c["dtype"]
        p = c["params"]
        args = (p.get("baud", 122.5), p.get("samp_rate", 96000))
        if c["status"] == "err":
            with pytest.raises(ValueError) as e:
                hc.demodulate(x, *args)
            assert c["etype"] == "ValueError" and str(e.value) == c["emsg"], c["id"]
        else:
            assert hc.demodulate(x, *args).hex() == c["out"], c["id"]
        n += 1
    assert n >= 20


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sps", SPS)
def test_restated_energies_equal_numpy_mean(sps, dtype):
    rng = np.random.default_rng(1000 * sps + len(dtype))
    n_pix = 200 if sps <= 1000 else 6
    x = draw(rng, dtype, n_pix * sps + 3)
    want = hc.numpy_energies(x, sps)
    got = hc.energies(x, sps)
    assert got.dtype == want.dtype and got.shape == want.shape == (n_pix,)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (sps, dtype)
    if np.dtype(dtype).kind == "f":
        # the case can tell the orders apart: a plain left-to-right sum in the
        # same dtype differs from np.mean on at least one pixel.  Below 8
        # samples numpy's order IS the serial one, so there the two must agree.
        # (float16: the plain sum also accumulates in float16, the array's own dtype.)
        if dtype == "float16":
            px = hc.pixels(x, sps)
            with np.errstate(all="ignore"):
                plain = (hc.serial_sum(px * px) / np.float16(sps)).astype(np.float16)
        else:
            plain = hc.energies(x, sps, summer=hc.serial_sum)
        if sps < 8 and dtype != "float16":
            assert np.array_equal(plain, want)
        else:
            assert np.any(plain != want), (sps, dtype)


def test_leaf_list_shape():
    """The tree the kernel's plan encodes: leaves of <= 128, each starting at a
    multiple of 8, only the last with a tail; 784 -> 96,96,96,104,96,96,96,104."""
    assert [m for _, m in hc.leaves(784)] == [96, 96, 96, 104, 96, 96, 96, 104]
    for n in (1, 7, 8, 128, 129, 136, 1000, 8191, 8192):
        lv = hc.leaves(n)
        assert sum(m for _, m in lv) == n and all(o % 8 == 0 and 0 < m <= 128 for o, m in lv)
        assert all(m % 8 == 0 for _, m in lv[:-1])
        assert all(m >= 64 for _, m in lv) or len(lv) == 1


def test_product_glyphs_equal_recorded_pixels(built_lib):
    import _amr
    rows = _amr.hell_glyph_rows()                      # [95][7] uint8 from libamr.so
    want = hc.glyph_rows()
    assert rows.shape == (95, 7) and len(want) == 95
    for i, (ch, rr) in enumerate(want.items()):
        assert ord(ch) == 0x20 + i
        assert rows[i].tolist() == rr, ch


def test_product_lookup_is_first_match_in_map_order(built_lib):
    import _amr
    lut = _amr.hell_rx_lookup()
    assert len(lut) == 128 and lut == hc.lookup_table()
    assert all(v == ord("?") for v in lut[32:])
    assert len({v for v in range(128) if any(v in rr for rr in hc.glyph_rows().values())}) == 30


def test_sps_zero_messages(built_lib, hell):
    """The reference's ValueErrors for sps == 0 come from host arithmetic in
    libamr.so, before any device work, with the reference's messages."""
    import modem
    cases, d = hell
    by = {c["id"]: c for c in cases}
    with pytest.raises(ValueError) as e:
        modem.feld_hell_demodulate(d["rx_sps0.in"], 200000, 1000.0)
    assert str(e.value) == by["rx_sps0"]["emsg"]
    with pytest.raises(ValueError) as e:
        modem.feld_hell_modulate(b"x", 200000, 1000.0)
    assert str(e.value) == by["tx_sps0"]["emsg"]
    with pytest.raises(ValueError) as e:
        modem.feld_hell_modulate(b"x", -9600, 1000.0)
    assert str(e.value) == by["tx_neg_baud"]["emsg"]
    with pytest.raises(ZeroDivisionError):
        modem.feld_hell_demodulate(d["rx_sps0.in"], 0, 1000.0)
    with pytest.raises(ZeroDivisionError):
        modem.feld_hell_modulate(b"x", 0, 1000.0)
    assert modem.feld_hell_demodulate(d["rx_neg_baud.in"], -9600, 1000.0) == b""      # negative step: no pixels


def test_unsupported_dtypes_name_themselves(built_lib):
    import modem
    for x in (np.zeros(2000, np.longdouble), np.zeros(2000, np.complex64), np.zeros(2000, object)):
        with pytest.raises(TypeError) as e:
            modem.feld_hell_demodulate(x, 122.5, 1000.0)
        assert str(x.dtype) in str(e.value)


def test_hellschreiber_mode_decodes_strictly():
    """encoder's HELLSCHREIBER mode passes framed.decode('utf-8') (encoder.py:196):
    a binary frame raises UnicodeDecodeError, as in the reference."""
    import encoder
    framed = encoder._frame_data("a.bin", b"\xff\xfe payload", 0, 1, 10, 0)
    with pytest.raises(UnicodeDecodeError):
        encoder._modulate_part(framed, "HELLSCHREIBER", 1200)


def test_no_gpu_is_an_error_not_a_fallback(built_lib):
    import _amr
    import modem
    if _amr.device_count() > 0:
        return                                          # the GPU suite covers the working path
    with pytest.raises(_amr.AmrError):
        modem.feld_hell_demodulate(np.zeros(8000, np.float32), 122.5, 1000.0)
    with pytest.raises(_amr.AmrError):
        modem.feld_hell_modulate(b"hi", 122.5, 1000.0)
