"""numpy restatement of minshift, the MSK modem of DESIGN §3m -- with that
section the specification: there is no reference for it, and the GPU must
reproduce these functions bit for bit, the transmit samples included (the sine
is the host's table).  Float64, no fma, every product rounded before it is
added; the samples as ofdm_cases.as_float64 reads them; the summation orders
are the loops below.

  geometry     _amr.msk_geometry: L samples per bit, h = L // 2, cyc4 quarter
               cycles of carrier per bit; design: _amr.design_msk's tables Sn,
               U, E0, E1, R (the same function the plan takes them from, so a
               table is never a source of difference)
  modulate     [0] + [1,0]*40 + payload bits + [0]; the integer phase p in units
               of 1 / (4 L) cycle: float32(Sn[(p_k + i * inc_k) % (4 L)]),
               inc_k = cyc4 + 1 for a 1 and cyc4 - 1 for a 0
  shift        spread_cases.shift
  windows      W[k] = sum_{i<L} shift(x, o)[(k+1) L - h + i] * U[i], k < Sw =
               max(0, (n + h) // L - 1): four interleaved partial sums p[i & 3],
               each sequential in i from 0.0, (p0 + p1) + (p2 + p3)
  products     D[k] = (W[k+1] * conj(W[k])) * (-i)^(cyc4 mod 4): numpy's complex
               multiply (the oracle's model), then a swap and negation
  slice_bits   1 iff D.imag > 0
  soft         soft_cases.psk_soft("bpsk", ...)'s magnitude rule with D.imag in
               the role of the real part; the hard bit's sign
  lines        c_t = sum_m (x[m] * x[m]) * E_t[m % (2 L)]: segments of 4096
               samples; in a segment partial j of 64 adds m = seg * 4096 + 64 a
               + j sequentially in a from 0.0; the partials by the tree j with
               j + 32, then 16, 8, 4, 2, 1; the segment sums in order from 0.0
  score        q = c1 * conj(c0) = (c1r c0r + c1i c0i, c1i c0r - c1r c0i),
               P[d] = q.re * R[d].re - q.im * R[d].im
  first_max    spread_cases.first_max
  demod        windows at the acquired (or zero) offset -> slice_bits -> sync search, pack
"""
from __future__ import annotations

import numpy as np

import _amr
import ofdm_cases as oc
import soft_cases as sc
import spread_cases as sp

PREAMBLE = [1, 0] * 40
SYNC_AT = 80                                                 # bit index of the payload's first bit
SEG = 4096
LANES = 64

shift = sp.shift
first_max = sp.first_max


def geometry(baud, carrier, samp_rate=96000):
    """(L, h, cyc4) or ValueError."""
    return _amr.msk_geometry(baud, carrier, samp_rate)


def pair_of(L: int, cyc4: int):
    """A (baud, carrier, samp_rate) that has the geometry (L, cyc4), every quotient exact."""
    baud, carrier, samp_rate = 1000, 250.0 * cyc4, 1000 * L
    assert geometry(baud, carrier, samp_rate)[::2] == (L, cyc4), (L, cyc4)
    return baud, carrier, samp_rate


def valid_pairs(max_L: int):
    """Every valid (L, cyc4) with 4 <= L <= max_L."""
    return [(L, c) for L in range(4, max_L + 1) for c in range(2, 2 * L - 1)]


def tx_bits(data: bytes) -> np.ndarray:
    return np.concatenate([np.zeros(1, np.uint8), np.array(PREAMBLE, np.uint8),
                           np.unpackbits(np.frombuffer(bytes(data), np.uint8)), np.zeros(1, np.uint8)])


def modulate(data: bytes, baud, carrier, samp_rate=96000) -> np.ndarray:
    L, h, cyc4, Sn, U, E0, E1, R = _amr.design_msk(baud, carrier, samp_rate)
    bits = tx_bits(data).astype(np.int64)
    inc = cyc4 + 2 * bits - 1
    p = np.zeros(bits.size, np.int64)
    for k in range(bits.size - 1):
        p[k + 1] = (p[k] + L * inc[k]) % (4 * L)
    idx = (p[:, None] + np.arange(L, dtype=np.int64)[None, :] * inc[:, None]) % (4 * L)
    return Sn[idx].astype(np.float32).ravel()


def n_windows(n: int, L: int) -> int:
    return max(0, (n + L // 2) // L - 1)


def windows(x, o, baud, carrier, samp_rate=96000) -> np.ndarray:
    """W [Sw] complex128 of one stream read from offset o."""
    L, h, cyc4, Sn, U, E0, E1, R = _amr.design_msk(baud, carrier, samp_rate)
    x = shift(oc.as_float64(x), int(o))
    S = n_windows(x.size, L)
    X = x[L - h:L - h + S * L].reshape(S, L)
    pr, pi = np.zeros((4, S)), np.zeros((4, S))
    with np.errstate(all="ignore"):
        for i in range(L):
            pr[i & 3] = pr[i & 3] + X[:, i] * U[i, 0]
            pi[i & 3] = pi[i & 3] + X[:, i] * U[i, 1]
        W = np.empty(S, np.complex128)                       # the components as they are: no complex arithmetic here
        W.real = (pr[0] + pr[1]) + (pr[2] + pr[3])
        W.imag = (pi[0] + pi[1]) + (pi[2] + pi[3])
    return W


def products(W, cyc4: int) -> np.ndarray:
    """D [Sw - 1]: the differential products turned back by the carrier's cyc4 quarter-turns (exact)."""
    d = sc.diff_products(W)
    dr, di = d.real.copy(), d.imag.copy()
    D = np.empty(d.size, np.complex128)
    r = cyc4 % 4
    if r == 0:
        D.real, D.imag = dr, di
    elif r == 1:
        D.real, D.imag = di, -dr
    elif r == 2:
        D.real, D.imag = -dr, -di
    else:
        D.real, D.imag = -di, dr
    return D


def bits_of_products(D) -> np.ndarray:
    """The bit rule, total: 1 iff D.imag > 0; NaN and zeros of either sign give 0."""
    with np.errstate(all="ignore"):
        return (np.asarray(D, np.complex128).imag > 0).astype(np.uint8)


def slice_bits(W, cyc4: int) -> np.ndarray:
    return bits_of_products(products(W, cyc4))


def soft_of_products(D) -> np.ndarray:
    D = np.asarray(D, np.complex128)
    a, b = D.imag.copy(), D.real.copy()                      # a in the role of psk_soft's real part
    with np.errstate(all="ignore"):
        m = sc.magnitude(np.abs(a), np.abs(a) + np.abs(b))
        hard = a > 0
    return np.where(hard, m, -m).astype(np.int8)


def soft(W, cyc4: int) -> np.ndarray:
    """The soft values of one stream's W: int8, Sw - 1."""
    return soft_of_products(products(W, cyc4))


def tree(p: np.ndarray) -> np.ndarray:
    """[..., 64] partial sums -> [...]: j with j + 32, then 16, 8, 4, 2, 1."""
    w = LANES // 2
    while w:
        p = p[..., :w] + p[..., w:2 * w]
        w //= 2
    return p[..., 0]


def segment_sums(x, baud, carrier, samp_rate=96000) -> np.ndarray:
    """[segments][4]: (c0.re, c0.im, c1.re, c1.im) of each segment of 4096 samples (none when n = 0)."""
    L, h, cyc4, Sn, U, E0, E1, R = _amr.design_msk(baud, carrier, samp_rate)
    x = oc.as_float64(x)
    n = x.size
    nseg = -(-n // SEG)
    with np.errstate(all="ignore"):
        sq = x * x                                           # the square rounded first
        r = np.arange(n) % (2 * L)
        v = np.stack([sq * E0[r, 0], sq * E0[r, 1], sq * E1[r, 0], sq * E1[r, 1]])
        # a partial that gets no term, or fewer, stays as it is: adding +0.0 to a sum that began at +0.0 changes nothing
        v = np.concatenate([v, np.zeros((4, nseg * SEG - n))], axis=1).reshape(4, nseg, SEG // LANES, LANES)
        p = np.zeros((4, nseg, LANES))
        for a in range(SEG // LANES):
            p = p + v[:, :, a, :]
        return np.ascontiguousarray(tree(p).T)


def lines(x, baud, carrier, samp_rate=96000):
    """(c0, c1) complex128: the segment sums added in order from 0.0."""
    g = segment_sums(x, baud, carrier, samp_rate)
    return lines_of_segments(g)


def lines_of_segments(g):
    c = np.zeros(4)
    with np.errstate(all="ignore"):
        for s in range(g.shape[0]):
            c = c + g[s]
    return complex(c[0], c[1]), complex(c[2], c[3])


def score(c0, c1, R):
    """(q, P [L]); the components by hand: no complex arithmetic."""
    with np.errstate(all="ignore"):
        qr = np.float64(c1.real) * np.float64(c0.real) + np.float64(c1.imag) * np.float64(c0.imag)
        qi = np.float64(c1.imag) * np.float64(c0.real) - np.float64(c1.real) * np.float64(c0.imag)
        P = qr * R[:, 0] - qi * R[:, 1]
    return complex(qr, qi), P


def offset_of(c0, c1, baud, carrier, samp_rate=96000):
    """(o, q) from given line sums (what amr_msk_offset_host computes, the sums as one segment)."""
    R = _amr.design_msk(baud, carrier, samp_rate)[7]
    c0, c1 = lines_of_segments(np.array([[c0.real, c0.imag, c1.real, c1.imag]]))
    q, P = score(c0, c1, R)
    return first_max(P), q


def acquire(x, baud, carrier, samp_rate=96000):
    """(o, q) of one stream."""
    R = _amr.design_msk(baud, carrier, samp_rate)[7]
    q, P = score(*lines(x, baud, carrier, samp_rate), R)
    return first_max(P), q


def sync_pack(bits: np.ndarray):
    return oc.sync_pack(bits)


def demod(x, baud, carrier, samp_rate=96000, acquire_=True):
    """(bytes, sync index or -1, o) of one stream."""
    o = acquire(x, baud, carrier, samp_rate)[0] if acquire_ else 0
    W = windows(x, o, baud, carrier, samp_rate)
    if W.size < 2:
        return b"", -1, o
    return (*sync_pack(slice_bits(W, geometry(baud, carrier, samp_rate)[2])), o)


def demod_soft(x, baud, carrier, samp_rate=96000, acquire_=True):
    """(bytes, soft int8, sync index or -1, o) of one stream."""
    o = acquire(x, baud, carrier, samp_rate)[0] if acquire_ else 0
    W = windows(x, o, baud, carrier, samp_rate)
    if W.size < 2:
        return b"", np.zeros(0, np.int8), -1, o
    return (*sc.align(soft(W, geometry(baud, carrier, samp_rate)[2])), o)


def delayed(msg: bytes, t: int, baud, carrier, tail=None, sigma=0.0, rng=None, samp_rate=96000):
    """A capture of `msg`: t zeros, the frame, `tail` zeros (default 2 L), float32; N(0, sigma^2) on all of it."""
    L = geometry(baud, carrier, samp_rate)[0]
    w = modulate(msg, baud, carrier, samp_rate)
    x = np.concatenate([np.zeros(t, np.float32), w, np.zeros(2 * L if tail is None else tail, np.float32)])
    if sigma:
        x = x + rng.normal(0.0, sigma, x.size).astype(np.float32)
    return x
