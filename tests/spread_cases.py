"""numpy restatement of spread, the direct-sequence DBPSK modem of DESIGN §3l --
with that section the specification: there is no reference for it, and the GPU
must reproduce these functions bit for bit, the transmit samples included (the
sine is the host's table).  Float64, no fma; the samples as
ofdm_cases.as_float64 reads them; the summation orders are the loops below.

  geometry     _amr.dsss_geometry: spc, L = C spc, cyc whole carrier cycles per
               bit; design: _amr.design_dsss's tables Wc, T, Sn, cs (the same
               function the plan takes them from, so a table is never a source
               of difference)
  modulate     [1,0]*40 + payload bits; s[0] = +1, s[k+1] = -s[k] on a 1;
               float32(s[k] * (sg[i] * Sn[i]))
  shift        shift(x, o)[i] = x[i + o] while i + o < n, else 0.0
  symbols      Y[s] over shift(x, o)[s*L + i] * T[i]: four interleaved partial
               sums p[i & 3], each sequential in i from 0.0, every product
               rounded before it is added, (p0 + p1) + (p2 + p3)
  slice_bits   1 iff the real part of Y[s+1] * conj(Y[s]) is below 0 (numpy's
               complex multiply, the oracle's model)
  soft         soft_cases.psk_soft("bpsk", Y)
  chip_sums    u[m] = sum_{i < spc} x[m + i] * Wc[(m + i) % L], sequential from 0.0
  energy       P[d] = sum_q g_q[d], g_q[d] = sum over the segment's 64 bits of
               |sum_j cs[j] u[d + s L + j spc]|^2, all sequential from 0.0
  first_max    best = 0; for d = 1 .. L - 1: if P[d] > P[best]: best = d
  demod        symbols at the acquired (or zero) offset -> slice_bits -> sync search, pack
"""
from __future__ import annotations

import numpy as np

import _amr
import ofdm_cases as oc
import soft_cases as sc

PREAMBLE = [1, 0] * 40
SYNC_AT = 80                                                 # bit index of the payload's first bit
Q = 64
CODE13 = [0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0]            # the Barker sequence of length 13


def code64() -> list:
    """A fixed, seeded 64-chip code (no property claimed but its length)."""
    return np.random.default_rng(64).integers(0, 2, 64).tolist()


def geometry(baud, carrier, code=None, samp_rate=96000):
    """(spc, L, cyc, code) or ValueError."""
    return _amr.dsss_geometry(baud, carrier, code, samp_rate)


def tx_bits(data: bytes) -> np.ndarray:
    return np.concatenate([np.array(PREAMBLE, np.uint8), np.unpackbits(np.frombuffer(bytes(data), np.uint8))])


def modulate(data: bytes, baud, carrier, code=None, samp_rate=96000) -> np.ndarray:
    spc, L, cyc, c, Wc, T, Sn, cs = _amr.design_dsss(baud, carrier, code, samp_rate)
    bits = tx_bits(data)
    s = np.ones(1 + bits.size)
    for k in range(bits.size):
        s[k + 1] = -s[k] if bits[k] else s[k]
    sg = cs[np.arange(L) // spc]
    return (s[:, None] * (sg * Sn)[None, :]).astype(np.float32).ravel()


def shift(x, o: int) -> np.ndarray:
    """x read from sample o >= 0 on, zeros past its end, the length kept."""
    x = np.asarray(x)
    out = np.zeros(x.size, x.dtype)
    if o < x.size:
        out[:x.size - o] = x[o:]
    return out


def symbols(x, o, baud, carrier, code=None, samp_rate=96000) -> np.ndarray:
    """Y [S] complex128 of one stream read from offset o."""
    spc, L, cyc, c, Wc, T, Sn, cs = _amr.design_dsss(baud, carrier, code, samp_rate)
    x = shift(oc.as_float64(x), int(o))
    S = x.size // L
    X = x[:S * L].reshape(S, L)
    pr, pi = np.zeros((4, S)), np.zeros((4, S))
    with np.errstate(all="ignore"):
        for i in range(L):
            pr[i & 3] = pr[i & 3] + X[:, i] * T[i, 0]
            pi[i & 3] = pi[i & 3] + X[:, i] * T[i, 1]
        Y = np.empty(S, np.complex128)                       # the components as they are: no complex arithmetic here
        Y.real = (pr[0] + pr[1]) + (pr[2] + pr[3])
        Y.imag = (pi[0] + pi[1]) + (pi[2] + pi[3])
    return Y


def bits_of_products(d) -> np.ndarray:
    """The bit rule, total: 1 iff dr < 0; NaN and zeros of either sign give 0."""
    with np.errstate(all="ignore"):
        return (np.asarray(d, np.complex128).real < 0).astype(np.uint8)


def slice_bits(Y) -> np.ndarray:
    return bits_of_products(sc.diff_products(Y))


def soft(Y) -> np.ndarray:
    """The soft values of one stream's Y: int8, S - 1."""
    return sc.psk_soft("bpsk", Y)


def chip_sums(x, baud, carrier, code=None, samp_rate=96000):
    """(ur, ui), each n - spc + 1 values (none when n < spc)."""
    spc, L, cyc, c, Wc, T, Sn, cs = _amr.design_dsss(baud, carrier, code, samp_rate)
    x = oc.as_float64(x)
    nu = max(0, x.size - spc + 1)
    k = np.arange(x.size) % L
    ur, ui = np.zeros(nu), np.zeros(nu)
    with np.errstate(all="ignore"):
        pr, pi = x * Wc[k, 0], x * Wc[k, 1]                  # every product rounded before it is added
        for i in range(spc if nu else 0):
            ur = ur + pr[i:i + nu]
            ui = ui + pi[i:i + nu]
    return ur, ui


def acq_bits(n: int, L: int) -> int:
    return (n - L + 1) // L if n >= 2 * L - 1 else 0


def energy(x, baud, carrier, code=None, samp_rate=96000) -> np.ndarray:
    """P [L] of one stream."""
    spc, L, cyc, c, Wc, T, Sn, cs = _amr.design_dsss(baud, carrier, code, samp_rate)
    n = np.asarray(x).size
    M = acq_bits(n, L)
    P = np.zeros(L)
    if M == 0:
        return P
    ur, ui = chip_sums(x, baud, carrier, code, samp_rate)
    d = np.arange(L)
    with np.errstate(all="ignore"):
        for s0 in range(0, M, Q):
            g = np.zeros(L)
            for s in range(s0, min(s0 + Q, M)):
                yr, yi = np.zeros(L), np.zeros(L)
                for j in range(c.size):
                    m = d + s * L + j * spc
                    yr = yr + cs[j] * ur[m]
                    yi = yi + cs[j] * ui[m]
                g = g + (yr * yr + yi * yi)
            P = P + g
    return P


def first_max(P) -> int:
    """The sequential rule, as written: a NaN P[0] keeps 0, a NaN elsewhere never wins."""
    best = 0
    for d in range(1, len(P)):
        if P[d] > P[best]:
            best = d
    return best


def acquire(x, baud, carrier, code=None, samp_rate=96000):
    """(o, P) of one stream."""
    P = energy(x, baud, carrier, code, samp_rate)
    return first_max(P), P


def sync_pack(bits: np.ndarray):
    return oc.sync_pack(bits)


def demod(x, baud, carrier, code=None, samp_rate=96000, acquire_=True):
    """(bytes, sync index or -1, o) of one stream."""
    o = acquire(x, baud, carrier, code, samp_rate)[0] if acquire_ else 0
    Y = symbols(x, o, baud, carrier, code, samp_rate)
    if Y.size < 2:
        return b"", -1, o
    return (*sync_pack(slice_bits(Y)), o)


def demod_soft(x, baud, carrier, code=None, samp_rate=96000, acquire_=True):
    """(bytes, soft int8, sync index or -1, o) of one stream."""
    o = acquire(x, baud, carrier, code, samp_rate)[0] if acquire_ else 0
    Y = symbols(x, o, baud, carrier, code, samp_rate)
    if Y.size < 2:
        return b"", np.zeros(0, np.int8), -1, o
    return (*sc.align(soft(Y)), o)


def delayed(msg: bytes, t: int, baud, carrier, code=None, tail=None, sigma=0.0, rng=None, samp_rate=96000):
    """A capture of `msg`: t zeros, the frame, `tail` zeros (default 2 L), float32; N(0, sigma^2) on all of it."""
    L = geometry(baud, carrier, code, samp_rate)[1]
    w = modulate(msg, baud, carrier, code, samp_rate)
    x = np.concatenate([np.zeros(t, np.float32), w, np.zeros(2 * L if tail is None else tail, np.float32)])
    if sigma:
        x = x + rng.normal(0.0, sigma, x.size).astype(np.float32)
    return x
