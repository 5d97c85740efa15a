"""numpy restatement of the star16 modem of DESIGN §3o -- with that section the
specification: there is no reference for it, and the GPU must reproduce
these functions bit for bit (the transmit samples up to sin's last ulp).

  modulate     [0,0,0,0]*30 + [1,1,1,0]*10 + payload bits, four per symbol
               (a, b2, b1, b0): the tribit steps the phase as d8psk's does
               (psk8_cases GRAY / STEP / INV_GRAY), a toggles the ring (outer
               before the first symbol; A = 1.0 outer, 0.5 inner); the carrier
               runs in absolute time under the parabolic envelope
               env[i] = 4.0 * (u * (1.0 - u)), u = (i + 0.5) / sps
  energies     e = sr*sr + si*si on the real and imaginary arrays: two rounded
               products and one rounded sum
  slice_bits   per product the ring bit (e1 > 2.0 e0) | (e0 > 2.0 e1), then
               d8psk's tribit of the differential product (psk8_cases.tribits)
  soft         four int8 per product, a b2 b1 b0: the hard bit's sign,
               soft_cases.magnitude of min(|e1 - 2 e0|, |e0 - 2 e1|) / (e0 + e1)
               for a, psk8_cases' three expressions for the rest
  demod        oracle.psk_symbols("qpsk", ...) -> slice_bits -> sync search, pack
  demod_soft   ... -> soft -> soft_cases.align
"""
from __future__ import annotations

import numpy as np

import psk8_cases as p8
import soft_cases as sc

PREAMBLE = [0, 0, 0, 0] * 30 + [1, 1, 1, 0] * 10
CONFIGS = p8.CONFIGS


def tx_bits(data: bytes) -> np.ndarray:
    """The transmitted bit string: 8 len(data) is a multiple of 4, so there is no padding."""
    return np.concatenate([np.array(PREAMBLE, np.uint8), np.unpackbits(np.frombuffer(bytes(data), np.uint8))])


def envelope(sps: int) -> np.ndarray:
    u = (np.arange(sps) + 0.5) / sps
    return 4.0 * (u * (1.0 - u))


def phases_amps(data: bytes):
    """(ph, A) per symbol: the phase summed sequentially in float64 from 0.0, the ring toggled by a."""
    b = tx_bits(data).reshape(-1, 4).astype(np.int64)
    g = 4 * b[:, 1] + 2 * b[:, 2] + b[:, 3]
    ph, amp = np.empty(g.size), np.empty(g.size)
    cur, ring = 0.0, 1
    for k, (a, m) in enumerate(zip(b[:, 0], p8.INV_GRAY[g])):
        cur = cur + float(p8.STEP[m]) * (np.pi / 4)
        ring ^= int(a)
        ph[k] = cur
        amp[k] = 1.0 if ring else 0.5
    return ph, amp


def modulate(data: bytes, baud=1200, carrier=3000.0, samp_rate=96000) -> np.ndarray:
    sps = int(samp_rate / baud)
    if sps < 1:
        raise ValueError("star16: fewer than one sample per symbol")
    ph, amp = phases_amps(data)
    n = np.arange(ph.size * sps)
    k, i = n // sps, n % sps
    env = envelope(sps)
    return (np.sin(((2 * np.pi) * carrier) * (n / samp_rate) + ph[k]) * (env[i] * amp[k])).astype(np.float32)


def energies(sym) -> np.ndarray:
    s = np.ascontiguousarray(sym, np.complex128).ravel()
    sr, si = s.real.copy(), s.imag.copy()
    with np.errstate(all="ignore"):
        return sr * sr + si * si


def ring_bits(e) -> np.ndarray:
    """a of each product from the symbols' energies: total (NaN, inf against inf, zeros and ties give 0)."""
    e = np.asarray(e, np.float64)
    with np.errstate(all="ignore"):
        return ((e[1:] > 2.0 * e[:-1]) | (e[:-1] > 2.0 * e[1:])).astype(np.int64)


def nibbles(sym) -> np.ndarray:
    return 8 * ring_bits(energies(sym)) + p8.tribits(sc.diff_products(sym))


def slice_bits(sym) -> np.ndarray:
    """The decided bits of one stream's symbols: uint8, 4 (S - 1), MSB first."""
    v = nibbles(sym)
    return ((v[:, None] >> np.array([3, 2, 1, 0])) & 1).astype(np.uint8).ravel()


def ring_soft(e) -> np.ndarray:
    """The signed soft value of a per product."""
    e = np.asarray(e, np.float64)
    e0, e1 = e[:-1], e[1:]
    with np.errstate(all="ignore"):
        p, r = np.abs(e1 - 2.0 * e0), np.abs(e0 - 2.0 * e1)
        m = sc.magnitude(np.where(p < r, p, r), e0 + e1)
    return np.where(ring_bits(e) != 0, m, -m).astype(np.int8)


def soft(sym) -> np.ndarray:
    """The soft values of one stream's symbols: int8, 4 (S - 1), in bit order a, b2, b1, b0."""
    d = sc.diff_products(sym)
    out = np.empty(4 * d.size, np.int8)
    out[0::4] = ring_soft(energies(sym))
    t = p8.soft_of_products(d)
    out[1::4], out[2::4], out[3::4] = t[0::3], t[1::3], t[2::3]
    return out


def symbols(x, baud, carrier=3000.0, samp_rate=96000, raw_int16=False) -> np.ndarray:
    return p8.symbols(x, baud, carrier, samp_rate, raw_int16)


def demod(x, baud, carrier=3000.0, samp_rate=96000, raw_int16=False):
    """(bytes, sync index or -1) of one stream."""
    sym = symbols(x, baud, carrier, samp_rate, raw_int16)
    if sym.size < 2:
        return b"", -1
    return p8.sync_pack(slice_bits(sym))


def demod_soft(x, baud, carrier=3000.0, samp_rate=96000, raw_int16=False):
    """(bytes, soft int8, sync index or -1) of one stream."""
    sym = symbols(x, baud, carrier, samp_rate, raw_int16)
    if sym.size < 2:
        return b"", np.zeros(0, np.int8), -1
    return sc.align(soft(sym))
