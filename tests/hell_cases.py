"""Our own restatement of the Hellschreiber receiver (hellschreiber.py:155-187)
for the tests: numpy's summation order written out, the dtype table, and the
7-pixel lookup built from the recorded glyph pixels (tests/golden/hell_glyphs.json).

Summation order of np.mean(chunk ** 2) (numpy's add.reduce inner loop):
  acc = 0; for each consecutive block of 8192 squares: acc = acc + pairwise(block)
  pairwise(a, n):  n < 8    serial from 0
                   n <= 128 r[k] = a[k]; r[k] += a[i + k] for i = 8, 16, ... < n - n % 8;
                            ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)); then the n % 8 tail serially
                   else     n2 = n // 2; n2 -= n2 % 8; pairwise(a, n2) + pairwise(a + n2, n - n2)
dtype table (square in / sum in / mean / compared against); the quotient
sum / np.intp(sps) is a float64 division in numpy 2 whatever the sum's dtype,
cast once to the result dtype:
  float32   float32 / float32 / float32(float64(sum) / sps)  / float32(0.1)
  float64   float64 / float64 / sum / sps                    / 0.1
  float16   float16 / float32 / float16(float64(sum) / sps)  / float16(0.1)
  integers  own dtype, wrapping / float64 / float64          / 0.1      (bool ** 2 is int8)
"""
from __future__ import annotations

import json
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK = 8192


def leaves(n: int):
    """The leaves of pairwise(a, n) in order: [(offset, length)], every length <= 128."""
    if n <= 128:
        return [(0, n)]
    n2 = n // 2
    n2 -= n2 % 8
    return leaves(n2) + [(n2 + o, m) for o, m in leaves(n - n2)]


def _pairwise(sq: np.ndarray):
    """pairwise(a, n) over the LAST axis of sq [..., n] (every row the same tree)."""
    n = sq.shape[-1]
    if n < 8:
        r = np.zeros(sq.shape[:-1], sq.dtype)
        for i in range(n):
            r = r + sq[..., i]
        return r
    if n <= 128:
        m = n - n % 8
        r = sq[..., 0:8].copy()
        for i in range(8, m, 8):
            r = r + sq[..., i:i + 8]
        res = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))
        for i in range(m, n):
            res = res + sq[..., i]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(sq[..., :n2]) + _pairwise(sq[..., n2:])


def blocked_sum(sq: np.ndarray):
    """numpy's add.reduce of sq [..., n] along the last axis, in sq's dtype."""
    acc = np.zeros(sq.shape[:-1], sq.dtype)
    for b0 in range(0, sq.shape[-1], BLOCK):
        acc = acc + _pairwise(sq[..., b0:b0 + BLOCK])
    return acc


def serial_sum(sq: np.ndarray):
    """The plain left-to-right sum in sq's dtype (what the order must NOT be)."""
    acc = np.zeros(sq.shape[:-1], sq.dtype)
    for i in range(sq.shape[-1]):
        acc = acc + sq[..., i]
    return acc


def squares(px: np.ndarray):
    """chunk ** 2 as numpy forms it, cast to the dtype np.mean accumulates in."""
    if px.dtype.kind == "b":
        px = px.astype(np.int8)
    with np.errstate(all="ignore"):
        sq = px * px                                    # integers wrap in their own dtype
    if px.dtype == np.float16:
        return sq.astype(np.float32)
    if px.dtype.kind in "iu":
        return sq.astype(np.float64)
    return sq


def mean_of(total: np.ndarray, sps: int, dtype):
    """np.mean's division and result dtype for an input of `dtype`."""
    dtype = np.dtype(dtype)
    with np.errstate(all="ignore"):
        # numpy 2: sum / np.intp(count) is a float64 division whatever the sum's
        # dtype; the quotient is then cast once to the result dtype
        q = total.astype(np.float64) / np.float64(sps)
        if dtype == np.float16:
            return q.astype(np.float16)
        if dtype == np.float32:
            return q.astype(np.float32)
        return q


def threshold(dtype):
    dtype = np.dtype(dtype)
    return dtype.type(0.1) if dtype.kind == "f" else np.float64(0.1)


def pixels(x: np.ndarray, sps: int) -> np.ndarray:
    """x [..., N] -> [..., N // sps, sps] (the tail dropped)."""
    n_pix = x.shape[-1] // sps
    return x[..., :n_pix * sps].reshape(x.shape[:-1] + (n_pix, sps))


def energies(x: np.ndarray, sps: int, summer=blocked_sum) -> np.ndarray:
    """np.mean(chunk ** 2) of every pixel of x [..., N], in np.mean's result dtype."""
    px = pixels(np.asarray(x), sps)
    dt = np.int8 if px.dtype.kind == "b" else px.dtype
    return mean_of(summer(squares(px)), sps, dt)


def numpy_energies(x: np.ndarray, sps: int) -> np.ndarray:
    """The direct cross-check: np.mean(chunk ** 2) pixel by pixel, as the reference calls it."""
    x = np.asarray(x)
    with np.errstate(all="ignore"):
        return np.array([np.mean(x[i:i + sps] ** 2) for i in range(0, x.size - sps + 1, sps)])


def glyph_pixels() -> dict:
    with open(os.path.join(G, "hell_glyphs.json")) as f:
        return json.load(f)["glyphs"]


def glyph_rows() -> dict:
    """char -> its 7 row values (bit i of a row = pixel i of the row, LSB sent first)."""
    return {ch: [sum(b << i for i, b in enumerate(px[7 * r:7 * r + 7])) for r in range(7)]
            for ch, px in glyph_pixels().items()}


def lookup_table() -> bytes:
    """128 bytes: the first character, in map order, with any row equal to v; else '?'."""
    rows = glyph_rows()
    lut = bytearray(b"?" * 128)
    for v in range(128):
        for ch, rr in rows.items():                     # json keeps the recorded (map) order
            if v in rr:
                lut[v] = ord(ch)
                break
    return bytes(lut)


def sps_of(baud, samp_rate) -> int:
    return int(round(samp_rate / baud))


def demodulate(x: np.ndarray, baud=122.5, samp_rate=96000, lut: bytes | None = None) -> bytes:
    """hellschreiber_demodulate(x, baud, _, samp_rate).encode() restated."""
    x = np.asarray(x)
    sps = sps_of(baud, samp_rate)
    if sps == 0:
        raise ValueError("range() arg 3 must not be zero")
    if sps < 0 or x.size < sps:
        return b""
    lut = lut or lookup_table()
    dt = np.int8 if x.dtype.kind == "b" else x.dtype
    with np.errstate(all="ignore"):
        bits = energies(x, sps) > threshold(dt)
    out = bytearray()
    for g in range(bits.size // 7):
        out.append(lut[sum(int(b) << i for i, b in enumerate(bits[7 * g:7 * g + 7]))])
    return bytes(out)
