#!/usr/bin/env python3
"""Generate the Hellschreiber fixtures by running the REFERENCE's hellschreiber.py
(needs the reference checkout that make_golden.py imports from; the tests need
only the committed data).

Committed output is data only:
  tests/golden/hell.npz            demodulator cases: the capture ("<id>.in", in
                                   the caller's dtype).  Modulator cases: the
                                   reference waveform in the lossless form
                                   pixel bits ("<id>.bits", uint8) x the one
                                   on-pixel row ("<id>.row", float32 [sps]) --
                                   every on-pixel of the reference's output is
                                   the same samples and every off-pixel zero,
                                   which this script asserts before it drops
                                   the full array -- and the same for the int16
                                   samples of the WAV the reference writes
                                   ("<id>.pcmrow").
  tests/golden/hell_manifest.json  per case: the reference call, its
                                   parameters, the output bytes (hex) or the
                                   exception type + message it raised
  tests/golden/hell_glyphs.json    for each printable ASCII character the 49
                                   pixel bits (7 rows x 7, in transmit order)
                                   read back from the reference modulator's
                                   output, plus the cell length it sends for a
                                   character outside its map

Reference calls (file:line in the reference tree):
  hellschreiber.hellschreiber_modulate     hellschreiber.py:109-152
  hellschreiber.hellschreiber_demodulate   hellschreiber.py:155-187
  modem.feld_hell_modulate / _demodulate   modem.py:400-403
  modem.wav_from_array                     modem.py:360-368

Run:  python tests/golden/make_hell_golden.py
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (reference import helper)


def main():
    scratch = tempfile.mkdtemp(prefix="amr_hell_golden_")
    cwd = os.getcwd()
    modem, _, _ = make_golden._import_reference(scratch)
    import hellschreiber as hs
    rng = np.random.default_rng(20261019)
    arrays = {}
    cases = []

    # ---- demodulator --------------------------------------------------------
    def add_rx(case_id, x, fn="hellschreiber_demodulate", **params):
        arrays[f"{case_id}.in"] = x
        rec = {"id": case_id, "kind": "rx", "fn": fn, "params": params, "dtype": str(x.dtype), "n": int(x.size)}
        try:
            if fn == "feld_hell_demodulate":
                out = modem.feld_hell_demodulate(x, params["baud"], params["carrier"], params["samp_rate"])
            else:
                out = hs.hellschreiber_demodulate(x, **params).encode("utf-8")
            rec.update(status="ok", out=bytes(out).hex())
        except Exception as e:          # the reference's error contract is part of parity
            rec.update(status="err", etype=type(e).__name__, emsg=str(e))
        cases.append(rec)

    def keyed(vals, sps, amp=0.9, fc=1000.0, fs=96000.0, tail=0):
        """On/off keyed tone: the 7-pixel groups spell the values `vals` (LSB first)."""
        bits = np.array([(v >> i) & 1 for v in vals for i in range(7)], np.float64)
        tone = amp * np.sin(2 * np.pi * fc * np.arange(sps) / fs)
        x = (bits[:, None] * tone[None, :]).ravel()
        return np.concatenate([x, np.zeros(tail)])

    def noisy(x, sigma):
        return x + rng.normal(0.0, sigma, x.size)

    vals = list(rng.permutation(128))
    # float32 / float64 at the default parameters (sps 784), the lookup's domain and beyond
    add_rx("rx_f32_default", noisy(keyed(vals[:5], 784, tail=100), 0.05).astype(np.float32))
    add_rx("rx_f64_default", noisy(keyed([1, 17, 4], 784), 0.05))
    # every 7-pixel value once, short pixels (sps 10), then near the threshold
    add_rx("rx_f32_all128", noisy(keyed(vals, 10, fc=12000.0, tail=7), 0.02).astype(np.float32), baud=9600)
    add_rx("rx_f32_edge", noisy(keyed(vals[:20], 100, amp=0.4472, fc=3000.0), 0.02).astype(np.float32), baud=960)
    add_rx("rx_f64_edge", noisy(keyed(vals[40:60], 100, amp=0.4472, fc=3000.0), 0.02), baud=960)
    add_rx("rx_f16_edge", noisy(keyed(vals[80:100], 100, amp=0.4472, fc=3000.0), 0.02).astype(np.float16), baud=960)
    add_rx("rx_f16_big", (300.0 * noisy(keyed(vals[:20], 9, fc=12000.0), 0.3)).astype(np.float16),
           baud=10666, samp_rate=96000)                                     # squares overflow float16
    # integers: raw values, the square wrapping in the array's own dtype
    add_rx("rx_i16_wrap", rng.integers(-32768, 32768, 7 * 30 * 9 + 4).astype(np.int16), baud=10666)
    add_rx("rx_i16_small", rng.integers(-1, 2, 7 * 30 * 9).astype(np.int16), baud=10666)
    add_rx("rx_u8", rng.integers(0, 256, 7 * 25 * 5 + 3).astype(np.uint8), baud=19200)
    add_rx("rx_u8_small", rng.integers(0, 2, 7 * 25 * 5).astype(np.uint8) * rng.integers(0, 2, 7 * 25 * 5).astype(np.uint8),
           baud=19200)
    add_rx("rx_i8", rng.integers(-128, 128, 7 * 25 * 5).astype(np.int8), baud=19200)
    add_rx("rx_i32", rng.integers(-70000, 70000, 7 * 6 * 128).astype(np.int32), baud=750)
    add_rx("rx_i64", rng.integers(-2**33, 2**33, 7 * 12 * 9).astype(np.int64), baud=10666)
    add_rx("rx_u16", rng.integers(0, 65536, 7 * 12 * 9).astype(np.uint16), baud=10666)
    add_rx("rx_u32", rng.integers(0, 2**32, 7 * 12 * 9).astype(np.uint32), baud=10666)
    add_rx("rx_u64", rng.integers(0, 2**63, 7 * 12 * 9).astype(np.uint64), baud=10666)
    add_rx("rx_bool", (rng.random(7 * 40 * 5) < 0.12), baud=19200)
    # long pixels: more than one 8192 block per pixel
    add_rx("rx_f32_sps8193", noisy(keyed([5], 8193, amp=0.45, fc=50.0, fs=8193.0), 0.02).astype(np.float32),
           baud=1, samp_rate=8193)
    # lengths around a pixel and a group
    add_rx("rx_short", noisy(keyed([127], 784), 0.01).astype(np.float32)[:783])
    add_rx("rx_one_pixel", noisy(keyed([127], 784), 0.01).astype(np.float32)[:784])
    add_rx("rx_six_pixels", noisy(keyed([127], 784), 0.01).astype(np.float32)[:7 * 784 - 1])
    add_rx("rx_empty", np.zeros(0, np.float32))
    # the alias, a non-default sample rate, the error contract
    add_rx("rx_alias_44k", noisy(keyed(vals[:9], 360, fs=44100.0), 0.05).astype(np.float32),
           fn="feld_hell_demodulate", baud=122.5, carrier=1000.0, samp_rate=44100)
    add_rx("rx_sps0", np.zeros(64, np.float32), baud=200000)
    add_rx("rx_neg_baud", np.ones(64, np.float32), baud=-9600)

    # ---- modulator ----------------------------------------------------------
    def add_tx(case_id, text, fn="hellschreiber_modulate", **params):
        rec = {"id": case_id, "kind": "tx", "fn": fn, "params": params}
        if fn == "feld_hell_modulate":
            rec["data"] = bytes(text).hex()
            call = lambda: modem.feld_hell_modulate(text, params["baud"], params["carrier"], params["samp_rate"])  # noqa: E731
        else:
            rec["text"] = text
            call = lambda: hs.hellschreiber_modulate(text, **params)  # noqa: E731
        try:
            out = call()
        except Exception as e:
            rec.update(status="err", etype=type(e).__name__, emsg=str(e))
            cases.append(rec)
            return
        out = np.asarray(out)
        sps = int(round(params.get("samp_rate", 96000) / params.get("baud", 122.5)))
        px = out.reshape(-1, sps)
        bits = np.any(px != 0, axis=1)
        wav = np.frombuffer(modem.wav_from_array(out), dtype=np.uint8)
        pcm = wav[44:].view(np.int16).reshape(-1, sps)
        if bits.any():
            row, pcmrow = px[np.argmax(bits)], pcm[np.argmax(bits)]
        else:                                           # carrier 0: an all-zero waveform; no on-pixel to keep
            row, pcmrow = np.zeros(sps, np.float32), np.zeros(sps, np.int16)
        assert np.array_equal(bits[:, None] * row[None, :], px) and np.array_equal(bits[:, None] * pcmrow[None, :], pcm)
        arrays[f"{case_id}.bits"] = bits.astype(np.uint8)
        arrays[f"{case_id}.row"] = row
        arrays[f"{case_id}.pcmrow"] = pcmrow
        rec.update(status="ok", dtype=str(out.dtype), n=int(out.size), sps=sps, wav_header=wav[:44].tobytes().hex())
        cases.append(rec)

    add_tx("tx_default", "CQ de K1ABC 73!")
    add_tx("tx_outofmap", "A\tbé~€ z\x7f")                      # tab, e-acute, euro sign, DEL: blank cells
    add_tx("tx_empty", "")
    add_tx("tx_carrier0", "HI", carrier=0.0)
    add_tx("tx_baud5", "5", baud=5)                                        # sps 19200
    add_tx("tx_fast", "The quick brown fox", baud=9600, carrier=12000.0)
    add_tx("tx_44k", "hell0 W0RLD", baud=245, carrier=980.0, samp_rate=44100)
    add_tx("tx_alias_bytes", b"ok \xff\xfe\xc3\xa9 {}", fn="feld_hell_modulate", baud=1200, carrier=3000.0,
           samp_rate=96000)                                                # invalid UTF-8 is ignored, e-acute is blank
    add_tx("tx_sps0", "x", baud=200000)
    add_tx("tx_neg_baud", "x", baud=-9600)

    # ---- glyph bitmaps, read back from the modulator's output ------------------
    glyphs = {}
    for code in range(0x20, 0x7F):
        out = hs.hellschreiber_modulate(chr(code), baud=9600)             # sps 10
        px = np.any(out.reshape(-1, 10) != 0, axis=1).astype(int)
        assert px.size == 70 + 51 + 35
        glyphs[chr(code)] = px[70:70 + 49].tolist()
        assert not px[70 + 49:70 + 51].any()
    blank = hs.hellschreiber_modulate("é", baud=9600)
    blank_px = np.any(blank.reshape(-1, 10) != 0, axis=1).astype(int)

    os.chdir(cwd)
    np.savez_compressed(os.path.join(HERE, "hell.npz"), **arrays)
    manifest = {"generator": "tests/golden/make_hell_golden.py",
                "reference": "szumanski/Audio-Modem-Radio",
                "numpy": np.__version__, "cases": cases}
    with open(os.path.join(HERE, "hell_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    with open(os.path.join(HERE, "hell_glyphs.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_hell_golden.py", "preamble_pixels": 70, "trailer_pixels": 35,
                   "blank_cell_pixels": int(blank_px.size - 105), "glyphs": glyphs}, f, indent=0)
    for c in cases:
        print(c["id"], c["status"], (c.get("out", "")[:40] or c.get("n")) if c["status"] == "ok" else c["emsg"][:80])


if __name__ == "__main__":
    main()
