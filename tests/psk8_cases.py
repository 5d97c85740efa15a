"""numpy restatement of the d8psk modem of DESIGN §3i -- with that section the
specification: there is no reference for it, and the GPU must reproduce
these functions bit for bit (the transmit samples up to sin's last ulp).

  modulate     [0,0,0]*30 + [1,1,0]*10 + payload bits, zero-padded to a
               multiple of 3; tribit g = GRAY[m] selects the phase step
               float(STEP[m]) * (pi / 4), summed sequentially in float64; the
               carrier runs in absolute time, the envelope is the PSK
               modulators' (all ones when the 10 % ramp is empty)
  slice_bits   the eight-sector decision on the differential products
               (soft_cases.diff_products: numpy's complex multiply), one
               rounded product T * x and one compare per test
  soft         three int8 per product, b2 b1 b0: the hard bit's sign,
               soft_cases.magnitude of the distance from the bit's decision lines
  demod        oracle.psk_symbols("qpsk", ...) -> slice_bits -> sync search, pack
  demod_soft   ... -> soft -> soft_cases.align
"""
from __future__ import annotations

import numpy as np

import soft_cases as sc

T = float.fromhex("0x1.a827999fcef32p-2")                  # the double nearest tan(pi / 8)
GRAY = np.array([0, 1, 3, 2, 6, 7, 5, 4])                    # phase-step index m -> tribit g = m ^ (m >> 1)
STEP = [0, 1, 2, 3, 4, -3, -2, -1]                           # m -> multiples of pi / 4 (the reference's -pi/2 for 270 deg)
INV_GRAY = np.argsort(GRAY)                                  # g -> m
PREAMBLE = [0, 0, 0] * 30 + [1, 1, 0] * 10
CONFIGS = [(1200, 3000.0), (2400, 3000.0), (4800, 12000.0), (9600, 12000.0), (19200, 24000.0)]   # (baud, carrier)


def tx_bits(data: bytes) -> np.ndarray:
    bits = np.concatenate([np.array(PREAMBLE, np.uint8), np.unpackbits(np.frombuffer(bytes(data), np.uint8))])
    return np.concatenate([bits, np.zeros(-bits.size % 3, np.uint8)])


def envelope(sps: int) -> np.ndarray:
    env = np.ones(sps)
    ramp = int(sps * 0.1)
    if ramp > 0:
        env[:ramp] = np.linspace(0, 1, ramp)
        env[-ramp:] = np.linspace(1, 0, ramp)
    return env


def phases(data: bytes) -> np.ndarray:
    b = tx_bits(data).reshape(-1, 3).astype(np.int64)
    g = 4 * b[:, 0] + 2 * b[:, 1] + b[:, 2]
    out = np.empty(g.size)
    ph = 0.0
    for k, m in enumerate(INV_GRAY[g]):
        ph = ph + float(STEP[m]) * (np.pi / 4)
        out[k] = ph
    return out


def modulate(data: bytes, baud=1200, carrier=3000.0, samp_rate=96000) -> np.ndarray:
    sps = int(samp_rate / baud)
    if sps < 1:
        raise ValueError("d8psk: fewer than one sample per symbol")
    ph = phases(data)
    n = np.arange(ph.size * sps)
    arg = ((2 * np.pi) * carrier) * (n / samp_rate) + ph[n // sps]
    return (np.sin(arg) * envelope(sps)[n % sps]).astype(np.float32)


def steps(d) -> np.ndarray:
    """The phase-step index m of each differential product."""
    d = np.asarray(d, np.complex128)
    dr, di = d.real, d.imag
    with np.errstate(all="ignore"):
        ar, ai = np.abs(dr), np.abs(di)
        axis_r = ai < T * ar
        axis_i = ar < T * ai
    diag = np.where(di > 0, np.where(dr > 0, 1, 3), np.where(dr > 0, 7, 5))
    return np.where(axis_r, np.where(dr > 0, 0, 4), np.where(axis_i, np.where(di > 0, 2, 6), diag))


def tribits(d) -> np.ndarray:
    return GRAY[steps(d)]


def slice_bits(sym) -> np.ndarray:
    """The decided bits of one stream's symbols: uint8, 3 (S - 1), one contiguous string."""
    g = tribits(sc.diff_products(sym))
    return ((g[:, None] >> np.array([2, 1, 0])) & 1).astype(np.uint8).ravel()


def soft_of_products(d) -> np.ndarray:
    d = np.asarray(d, np.complex128)
    dr, di = d.real.copy(), d.imag.copy()
    g = tribits(d)
    with np.errstate(all="ignore"):
        den = np.abs(dr) + np.abs(di)
        tr, ti = T * dr, T * di
        a, b = np.abs(di - tr), np.abs(dr + ti)
        m2 = sc.magnitude(np.abs(di + tr), den)
        m1 = sc.magnitude(np.abs(ti - dr), den)
        m0 = sc.magnitude(np.where(a < b, a, b), den)
    out = np.empty(3 * d.size, np.int8)
    out[0::3] = np.where(g & 4, m2, -m2)
    out[1::3] = np.where(g & 2, m1, -m1)
    out[2::3] = np.where(g & 1, m0, -m0)
    return out


def soft(sym) -> np.ndarray:
    """The soft values of one stream's symbols: int8, 3 (S - 1), in bit order b2, b1, b0."""
    return soft_of_products(sc.diff_products(sym))


def symbols(x, baud, carrier=3000.0, samp_rate=96000, raw_int16=False) -> np.ndarray:
    from oracle import oracle
    return oracle.psk_symbols("qpsk", x, baud, carrier, samp_rate, raw_int16=raw_int16)


def sync_pack(bits: np.ndarray):
    """(bytes, sync index or -1): the sync search and byte pack every PSK demodulator ends with."""
    sync = bits.tobytes().find(sc.SYNC_BITS)
    start = max(sync, 0)
    nb = (bits.size - start) // 8
    return np.packbits(bits[start:start + 8 * nb]).tobytes(), sync


def demod(x, baud, carrier=3000.0, samp_rate=96000, raw_int16=False):
    """(bytes, sync index or -1) of one stream."""
    sym = symbols(x, baud, carrier, samp_rate, raw_int16)
    if sym.size < 2:
        return b"", -1
    return sync_pack(slice_bits(sym))


def demod_soft(x, baud, carrier=3000.0, samp_rate=96000, raw_int16=False):
    """(bytes, soft int8, sync index or -1) of one stream."""
    sym = symbols(x, baud, carrier, samp_rate, raw_int16)
    if sym.size < 2:
        return b"", np.zeros(0, np.int8), -1
    return sc.align(soft(sym))
