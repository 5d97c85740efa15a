"""numpy restatement of tone8, the 8-FSK modem with Costas sync of DESIGN §3n
-- with that section the specification: there is no reference for it, and the
GPU must reproduce these functions bit for bit, the transmit samples included
(the sine is the host's table).  Float64, no fma, every product rounded before
it is added; the samples as ofdm_cases.as_float64 reads them; the summation
orders are the loops below.

  geometry     _amr.tone8_geometry: L samples per symbol, T = L // 8 per time
               slot, c2 half-cycles of carrier per symbol (tone m has c2 + 2 m),
               G half tone spacings searched either way; design:
               _amr.design_tone8's tables Sn, E (the same function the plan
               takes them from, so a table is never a source of difference)
  modulate     the Costas block 3, 1, 4, 0, 6, 5, 2, then the payload's tribits
               (MSB first, zero-padded), tribit v on tone v ^ (v >> 1); the
               integer phase p in units of 1 / (2 L) cycle:
               float32(Sn[(p_k + i * inc_k) % (2 L)]), inc_k = c2 + 2 tone_k
  slot_sums    Z[j][f] = sum_{i<T} x[j T + i] * E[(f (j T + i)) % (2 L)],
               sequential in i from 0.0, f = c2 - G .. c2 + 14 + G, j < J = n // T
  windows      Wd[j] = ((Z[j] + Z[j+1]) + (Z[j+2] + Z[j+3])) + ((Z[j+4] + Z[j+5])
               + (Z[j+6] + Z[j+7])), j < J - 7; P = re * re + im * im
  scores       S[j][g] = sum over s = 0..6 in order from 0.0 of
               P[j + 8 s][c2 + g + 2 costas[s]], j < nj = J - 55, g = -G .. G
  first_max    j ascending, g ascending within a j, strictly greater wins: a NaN
               never wins, a NaN first candidate keeps (0, -G)
  symbols      Y[k][m] = sum_{i<L} shift(x, o)[k L + i] * E[((c2 + g + 2 m) i) % (2 L)]:
               four interleaved partial sums p[i & 3], each sequential in i
               from 0.0, (p0 + p1) + (p2 + p3)
  decide       the first maximum of e_m = re * re + im * im from m = 0; the
               inverse Gray map, MSB first
  soft         a1 / a0 the largest e_m among the four tones whose tribit has the
               bit set / clear, folded in tone order, a NaN losing;
               soft_cases.magnitude(|a1 - a0|, a1 + a0); the hard bit's sign
  demod        symbols at the acquired (start % L, shift) or (0, 0) -> decide -> sync search, pack
"""
from __future__ import annotations

import numpy as np

import _amr
import ofdm_cases as oc
import soft_cases as sc
import spread_cases as sp

COSTAS = np.array(_amr.TONE8_COSTAS, np.int64)
SYNC_AT = 21                                                 # bit index of the payload's first bit
SPAN = 48                                                    # slots from the first Costas window to the last
AHEAD = 55                                                   # slots a start slot needs beyond itself
GRAY = np.array([v ^ (v >> 1) for v in range(8)], np.int64)                  # tribit -> tone
UNGRAY = np.array([t ^ (t >> 1) ^ (t >> 2) for t in range(8)], np.int64)     # tone -> tribit

shift = sp.shift


def geometry(baud, carrier, samp_rate=96000, search=6):
    """(L, T, c2, G) or ValueError."""
    return _amr.tone8_geometry(baud, carrier, samp_rate, search)


def pair_of(L: int, c2: int):
    """A (baud, carrier, samp_rate) that has the geometry (L, c2), every quotient exact."""
    baud, carrier, samp_rate = 1000, 500.0 * c2, 1000 * L
    assert geometry(baud, carrier, samp_rate, 0)[::2] == (L, c2), (L, c2)
    return baud, carrier, samp_rate


def valid_pairs(max_L: int):
    """Every valid (L, c2) at G = 0 with L <= max_L."""
    return [(L, c) for L in range(8, max_L + 1, 8) for c in range(2, L - 14)]


def tx_tones(data: bytes) -> np.ndarray:
    bits = np.unpackbits(np.frombuffer(bytes(data), np.uint8))
    bits = np.concatenate([bits, np.zeros(-bits.size % 3, np.uint8)]).reshape(-1, 3).astype(np.int64)
    v = 4 * bits[:, 0] + 2 * bits[:, 1] + bits[:, 2]
    return np.concatenate([COSTAS, GRAY[v]])


def modulate(data: bytes, baud, carrier, samp_rate=96000) -> np.ndarray:
    L, T, c2, G, Sn, E = _amr.design_tone8(baud, carrier, samp_rate, 0)
    inc = c2 + 2 * tx_tones(data)
    p = np.zeros(inc.size, np.int64)
    for k in range(inc.size - 1):
        p[k + 1] = (p[k] + L * inc[k]) % (2 * L)
    idx = (p[:, None] + np.arange(L, dtype=np.int64)[None, :] * inc[:, None]) % (2 * L)
    return Sn[idx].astype(np.float32).ravel()


def slot_sums(x, baud, carrier, samp_rate=96000, search=6):
    """(Zr, Zi) [J][NB]: the slot sums' components."""
    L, T, c2, G, Sn, E = _amr.design_tone8(baud, carrier, samp_rate, search)
    x = oc.as_float64(x)
    J = x.size // T
    f = np.arange(c2 - G, c2 + 15 + G, dtype=np.int64)
    X = x[:J * T].reshape(J, T)
    m0 = np.arange(J, dtype=np.int64) * T
    zr, zi = np.zeros((J, f.size)), np.zeros((J, f.size))
    with np.errstate(all="ignore"):
        for i in range(T):
            idx = (f[None, :] * (m0 + i)[:, None]) % (2 * L)
            zr = zr + X[:, i, None] * E[idx, 0]
            zi = zi + X[:, i, None] * E[idx, 1]
    return zr, zi


def window_energies(zr, zi) -> np.ndarray:
    """P [max(0, J - 7)][NB]."""
    nw = max(0, zr.shape[0] - 7)

    def tree(z):
        s = [z[k:k + nw] for k in range(8)]
        return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))
    with np.errstate(all="ignore"):
        re, im = tree(zr), tree(zi)
        return re * re + im * im


def scores(P, G: int) -> np.ndarray:
    """S [max(0, n_win - 48)][2 G + 1] from P [n_win][15 + 2 G]."""
    nj = max(0, P.shape[0] - SPAN)
    S = np.zeros((nj, 2 * G + 1))
    with np.errstate(all="ignore"):
        for s in range(7):
            S = S + P[8 * s:8 * s + nj, 2 * COSTAS[s]:2 * COSTAS[s] + 2 * G + 1]
    return S


def first_max_flat(v) -> int:
    """spread_cases.first_max's result without the loop: a NaN v[0] keeps 0; otherwise the first index of
    the greatest value that is not a NaN."""
    v = np.asarray(v, np.float64).ravel()
    if v.size == 0 or np.isnan(v[0]):
        return 0
    return int(np.argmax(np.where(np.isnan(v), -np.inf, v)))


def peak(P, T: int, G: int):
    """(start, shift, score) from given window energies (what amr_tone8_peak_host computes)."""
    S = scores(np.asarray(P, np.float64), G)
    if S.shape[0] == 0:
        return 0, 0, 0.0
    k = first_max_flat(S)
    j, gi = divmod(k, 2 * G + 1)
    return j * T, gi - G, float(S[j, gi])


def acquire(x, baud, carrier, samp_rate=96000, search=6):
    """(start, shift, score) of one stream."""
    L, T, c2, G = geometry(baud, carrier, samp_rate, search)
    return peak(window_energies(*slot_sums(x, baud, carrier, samp_rate, search)), T, G)


def symbols(x, o, g, baud, carrier, samp_rate=96000, search=6) -> np.ndarray:
    """Y [S][8] complex128 of one stream read from offset o with the tones moved by g."""
    L, T, c2, G, Sn, E = _amr.design_tone8(baud, carrier, samp_rate, search)
    assert 0 <= o < L and -G <= g <= G
    x = shift(oc.as_float64(x), int(o))
    S = x.size // L
    X = x[:S * L].reshape(S, L)
    inc = c2 + int(g) + 2 * np.arange(8, dtype=np.int64)
    pr, pi = np.zeros((4, S, 8)), np.zeros((4, S, 8))
    with np.errstate(all="ignore"):
        for i in range(L):
            idx = (inc * i) % (2 * L)
            pr[i & 3] = pr[i & 3] + X[:, i, None] * E[idx, 0]
            pi[i & 3] = pi[i & 3] + X[:, i, None] * E[idx, 1]
        Y = np.empty((S, 8), np.complex128)                  # the components as they are: no complex arithmetic here
        Y.real = (pr[0] + pr[1]) + (pr[2] + pr[3])
        Y.imag = (pi[0] + pi[1]) + (pi[2] + pi[3])
    return Y


def energies(Y) -> np.ndarray:
    Y = np.asarray(Y, np.complex128)
    with np.errstate(all="ignore"):
        return Y.real * Y.real + Y.imag * Y.imag


def decide(Y) -> np.ndarray:
    """The tone of each symbol [S]: best = 0; for m = 1 .. 7: if e[m] > e[best]: best = m."""
    e = energies(Y).reshape(-1, 8)
    best = np.zeros(e.shape[0], np.int64)
    bv = e[:, 0].copy()
    with np.errstate(all="ignore"):
        for m in range(1, 8):
            win = e[:, m] > bv
            bv = np.where(win, e[:, m], bv)
            best = np.where(win, m, best)
    return best


def slice_bits(Y) -> np.ndarray:
    """The 3 S decided bits, MSB first."""
    v = UNGRAY[decide(Y)]
    return np.stack([(v >> 2) & 1, (v >> 1) & 1, v & 1], axis=-1).astype(np.uint8).ravel()


def larger(a, b):
    """The larger of two energies, a NaN losing: b when it is greater or a is a NaN."""
    with np.errstate(all="ignore"):
        return np.where((b > a) | np.isnan(a), b, a)


def soft(Y) -> np.ndarray:
    """The soft values of one stream's Y: int8, 3 S."""
    e = energies(Y).reshape(-1, 8)
    hard = slice_bits(Y).reshape(-1, 3)
    out = np.empty((e.shape[0], 3), np.int8)
    for r in range(3):
        a = [None, None]
        for m in range(8):
            b = int(UNGRAY[m] >> (2 - r)) & 1
            a[b] = e[:, m] if a[b] is None else larger(a[b], e[:, m])
        with np.errstate(all="ignore"):
            mag = sc.magnitude(np.abs(a[1] - a[0]), a[1] + a[0])
        out[:, r] = np.where(hard[:, r] == 1, mag, -mag)
    return out.ravel()


def sync_pack(bits: np.ndarray):
    return oc.sync_pack(bits)


def where(x, baud, carrier, samp_rate=96000, acquire_=True, search=6):
    """(start, shift) the demodulation reads the stream at."""
    return acquire(x, baud, carrier, samp_rate, search)[:2] if acquire_ else (0, 0)


def demod(x, baud, carrier, samp_rate=96000, acquire_=True, search=6):
    """(bytes, sync index or -1, start, shift) of one stream."""
    L = geometry(baud, carrier, samp_rate, search)[0]
    start, g = where(x, baud, carrier, samp_rate, acquire_, search)
    Y = symbols(x, start % L, g, baud, carrier, samp_rate, search)
    if Y.shape[0] < 1:
        return b"", -1, start, g
    return (*sync_pack(slice_bits(Y)), start, g)


def demod_soft(x, baud, carrier, samp_rate=96000, acquire_=True, search=6):
    """(bytes, soft int8, sync index or -1, start, shift) of one stream."""
    L = geometry(baud, carrier, samp_rate, search)[0]
    start, g = where(x, baud, carrier, samp_rate, acquire_, search)
    Y = symbols(x, start % L, g, baud, carrier, samp_rate, search)
    if Y.shape[0] < 1:
        return b"", np.zeros(0, np.int8), -1, start, g
    return (*sc.align(soft(Y)), start, g)


def delayed(msg: bytes, t: int, baud, carrier, tail=None, sigma=0.0, rng=None, samp_rate=96000, off=0):
    """A capture of `msg`: t zeros, the frame, `tail` zeros (default 2 L), float32; N(0, sigma^2) on all of it.
    off: the sender's carrier in half tone spacings above the receiver's `carrier`."""
    L = geometry(baud, carrier, samp_rate, 0)[0]
    w = modulate(msg, baud, carrier + off * baud / 2, samp_rate)
    x = np.concatenate([np.zeros(t, np.float32), w, np.zeros(2 * L if tail is None else tail, np.float32)])
    if sigma:
        x = x + rng.normal(0.0, sigma, x.size).astype(np.float32)
    return x
