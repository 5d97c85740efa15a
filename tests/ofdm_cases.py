"""numpy restatement of the ofdm modem of DESIGN §3j -- with that section the
specification: there is no reference for it, and the GPU must reproduce
these functions bit for bit (the transmit samples up to sin's last ulp).

  geometry     _amr.ofdm_geometry: sps, L = K sps, Ncp = L // 8, Nu = L - Ncp,
               bins[k] = c0 - K // 2 + k; design: _amr.design_ofdm's table W
               (the same function the plan takes it from, so the table is
               never a source of difference)
  modulate     [0,0]*30 + [1,1]*10 + payload bits, zero-padded to a multiple
               of 2 K; dibit j on symbol 1 + j // K, subcarrier j % K; symbol 0
               the Newman phases (pi * (k*k)) / K; ph[s] = ph[s-1] + step in
               float64; K sines per sample summed sequentially in k from 0.0
  symbols      Y[s][k] over x[s*L + Ncp + m]: four interleaved partial sums
               p[m & 3], each sequential in m from 0.0, every product rounded
               before it is added, (p0 + p1) + (p2 + p3)
  slice_bits   the four-sector decision on Y[s+1][k] * conj(Y[s][k]) (numpy's
               complex multiply, the oracle's model), in dibit order j = s*K + k
  soft         two int8 per product: the hard bit's sign, K4s's magnitudes
  demod        symbols -> slice_bits -> sync search, pack
  demod_soft   ... -> soft -> soft_cases.align
"""
from __future__ import annotations

import numpy as np

import _amr
import soft_cases as sc

PREAMBLE = [0, 0] * 30 + [1, 1] * 10
CONFIGS = [(1200, 3000.0), (2400, 3000.0), (4800, 12000.0), (9600, 12000.0), (19200, 24000.0)]   # (baud, carrier)
STEPS = np.array([0.0, np.pi / 2, -np.pi / 2, np.pi])       # dibit 00, 01, 10, 11 -> phase step (the reference's QPSK map)
DIBIT = np.array([0, 1, 3, 2])                               # sector m -> dibit
SYNC_AT = 80                                                 # bit index of the payload's first bit


def geometry(baud, carrier, K, samp_rate=96000):
    """(sps, L, Ncp, Nu, bins) or ValueError."""
    return _amr.ofdm_geometry(baud, carrier, K, samp_rate)


def valid(baud, carrier, K, samp_rate=96000) -> bool:
    try:
        geometry(baud, carrier, K, samp_rate)
    except ValueError:
        return False
    return True


def tx_bits(data: bytes, K: int) -> np.ndarray:
    bits = np.concatenate([np.array(PREAMBLE, np.uint8), np.unpackbits(np.frombuffer(bytes(data), np.uint8))])
    return np.concatenate([bits, np.zeros(-bits.size % (2 * K), np.uint8)])


def n_symbols(n_bytes: int, K: int) -> int:
    return 1 + -(-(40 + 4 * n_bytes) // K)


def phases(data: bytes, K: int) -> np.ndarray:
    """ph [S][K]: the reference symbol, then one sequential float64 sum per subcarrier."""
    b = tx_bits(data, K).reshape(-1, 2).astype(np.int64)
    d = (2 * b[:, 0] + b[:, 1]).reshape(-1, K)
    k = np.arange(K)
    ph = np.empty((1 + d.shape[0], K))
    ph[0] = (np.pi * (k * k)) / K
    for s in range(d.shape[0]):
        ph[s + 1] = ph[s] + STEPS[d[s]]
    return ph


def modulate(data: bytes, baud, carrier, K, samp_rate=96000) -> np.ndarray:
    sps, L, Ncp, Nu, bins = geometry(baud, carrier, K, samp_rate)
    ph = phases(data, K)
    m = (np.arange(L) - Ncp) % Nu
    acc = np.zeros((ph.shape[0], L))
    for k in range(K):
        r = (int(bins[k]) * m) % Nu
        acc = acc + np.sin(((2 * np.pi) * (r / Nu))[None, :] + ph[:, k][:, None])
    return (acc * (1.0 / K)).astype(np.float32).ravel()


def as_float64(x) -> np.ndarray:
    """The samples as the front end reads them: int16 is PCM, x / 32768.0."""
    x = np.asarray(x)
    return x / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)


def symbols(x, baud, carrier, K, samp_rate=96000) -> np.ndarray:
    """Y [S][K] complex128 of one stream."""
    sps, L, Ncp, Nu, bins, W = _amr.design_ofdm(baud, carrier, K, samp_rate)
    x = as_float64(x)
    S = x.size // L
    X = x[:S * L].reshape(S, L)[:, Ncp:]
    pr = np.zeros((4, S, K))
    pi = np.zeros((4, S, K))
    with np.errstate(all="ignore"):
        for m in range(Nu):
            xm = X[:, m][:, None]
            pr[m & 3] = pr[m & 3] + xm * W[None, :, m, 0]
            pi[m & 3] = pi[m & 3] + xm * W[None, :, m, 1]
        Y = np.empty((S, K), np.complex128)                  # the components as they are: no complex arithmetic here
        Y.real = (pr[0] + pr[1]) + (pr[2] + pr[3])
        Y.imag = (pi[0] + pi[1]) + (pi[2] + pi[3])
    return Y


def products(Y) -> np.ndarray:
    """Y[s+1][k] * conj(Y[s][k]) in dibit order, as numpy's complex multiply evaluates it (the oracle's model)."""
    from oracle import oracle
    Y = np.asarray(Y, np.complex128)
    if Y.shape[0] < 2:
        return np.zeros(0, np.complex128)
    z, w = np.ascontiguousarray(Y[1:].ravel()), np.ascontiguousarray(np.conj(Y[:-1]).ravel())
    ab, mul = np.empty(z.size), np.empty(z.size, np.complex128)
    oracle.lib().oracle_np_complex_model(oracle._p(z), oracle._p(w), z.size, oracle._p(ab), oracle._p(mul))
    return mul


def sectors(d) -> np.ndarray:
    """The sector m of each product; zeros, NaN and exact ties fall to the second line."""
    d = np.asarray(d, np.complex128)
    dr, di = d.real, d.imag
    with np.errstate(all="ignore"):
        on_real = np.abs(di) < np.abs(dr)
    return np.where(on_real, np.where(dr > 0, 0, 2), np.where(di > 0, 1, 3))


def dibits(d) -> np.ndarray:
    return DIBIT[sectors(d)]


def bits_of_products(d) -> np.ndarray:
    g = dibits(d)
    return ((g[:, None] >> np.array([1, 0])) & 1).astype(np.uint8).ravel()


def slice_bits(Y) -> np.ndarray:
    """The decided bits of one stream's Y: uint8, 2 K (S - 1), one contiguous string."""
    return bits_of_products(products(Y))


def soft_of_products(d) -> np.ndarray:
    d = np.asarray(d, np.complex128)
    dr, di = d.real.copy(), d.imag.copy()
    g = dibits(d)
    with np.errstate(all="ignore"):
        den = np.abs(dr) + np.abs(di)
        mh = sc.magnitude(np.abs(dr + di), den)
        ml = sc.magnitude(np.abs(dr - di), den)
    out = np.empty(2 * d.size, np.int8)
    out[0::2] = np.where(g & 2, mh, -mh)
    out[1::2] = np.where(g & 1, ml, -ml)
    return out


def soft(Y) -> np.ndarray:
    """The soft values of one stream's Y: int8, 2 K (S - 1)."""
    return soft_of_products(products(Y))


def sync_pack(bits: np.ndarray):
    """(bytes, sync index or -1): the sync search and byte pack every PSK demodulator ends with."""
    sync = bits.tobytes().find(sc.SYNC_BITS)
    start = max(sync, 0)
    nb = (bits.size - start) // 8
    return np.packbits(bits[start:start + 8 * nb]).tobytes(), sync


def demod(x, baud, carrier, K, samp_rate=96000):
    """(bytes, sync index or -1) of one stream."""
    Y = symbols(x, baud, carrier, K, samp_rate)
    if Y.shape[0] < 2:
        return b"", -1
    return sync_pack(slice_bits(Y))


def demod_soft(x, baud, carrier, K, samp_rate=96000):
    """(bytes, soft int8, sync index or -1) of one stream."""
    Y = symbols(x, baud, carrier, K, samp_rate)
    if Y.shape[0] < 2:
        return b"", np.zeros(0, np.int8), -1
    return sc.align(soft(Y))
