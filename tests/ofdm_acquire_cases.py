"""numpy restatement of ofdm acquisition -- with that section the
specification: there is no reference for it, and the GPU must reproduce these
functions bit for bit.  Float64, no fma; the samples as ofdm_cases.as_float64
reads them; the summation orders are the loops below.

  fold       M = (n - Nu) // L periods (0 when n < Nu + L) in segments of Q = 64:
             g_q[r] sequential over its periods from 0.0 of d * d,
             d = x[s L + r] - x[s L + r + Nu];  G = g_0 + g_1 + ... from 0.0
  window     E[d] = G[d] + G[(d + 1) % L] + ... : Ncp terms, sequential from 0.0
  first_min  best = 0; for d = 1 .. L - 1: if E[d] < E[best]: best = d
  back_off   o = dhat - Ncp // 2; if o > L - 1 - Ncp: o -= L
  shift      shift(x, o)[i] = x[i + o] where 0 <= i + o < n, else 0.0
  demod      ofdm_cases.demod(shift(x, o)): the acquired demodulation
"""
from __future__ import annotations

import numpy as np

import ofdm_cases as oc

Q = 64


def periods(n: int, L: int, Nu: int) -> int:
    return (n - Nu) // L if n >= Nu + L else 0


def fold(x, L: int, Nu: int) -> np.ndarray:
    """G [L] of one stream."""
    x = oc.as_float64(x)
    M = periods(x.size, L, Nu)
    G = np.zeros(L)
    with np.errstate(all="ignore"):
        for s0 in range(0, M, Q):
            g = np.zeros(L)
            for s in range(s0, min(s0 + Q, M)):
                d = x[s * L:s * L + L] - x[s * L + Nu:s * L + Nu + L]
                g = g + d * d
            G = G + g
    return G


def window(G, Ncp: int) -> np.ndarray:
    """E [L]: Ncp consecutive values of G (cyclically) from each d on."""
    G = np.asarray(G, np.float64)
    L = G.size
    E = np.zeros(L)
    d = np.arange(L)
    with np.errstate(all="ignore"):
        for i in range(Ncp):
            E = E + G[(d + i) % L]
    return E


def first_min(E) -> int:
    """The sequential rule, as written: a NaN E[0] keeps 0, a NaN elsewhere never wins."""
    best = 0
    for d in range(1, len(E)):
        if E[d] < E[best]:
            best = d
    return best


def back_off(dhat: int, L: int, Ncp: int) -> int:
    o = dhat - Ncp // 2
    if o > L - 1 - Ncp:
        o -= L
    return o


def shift(x, o: int) -> np.ndarray:
    """x read from sample o on, zeros outside it, the length kept."""
    x = np.asarray(x)
    n = x.size
    out = np.zeros(n, x.dtype)
    lo, hi = max(0, -o), min(n, n - o)
    if hi > lo:
        out[lo:hi] = x[lo + o:hi + o]
    return out


def acquire(x, baud, carrier, K, samp_rate=96000):
    """(o, dhat, E) of one stream."""
    sps, L, Ncp, Nu, bins = oc.geometry(baud, carrier, K, samp_rate)
    E = window(fold(x, L, Nu), Ncp)
    dhat = first_min(E)
    return back_off(dhat, L, Ncp), dhat, E


def symbols_at(x, o: int, baud, carrier, K, samp_rate=96000) -> np.ndarray:
    return oc.symbols(shift(x, o), baud, carrier, K, samp_rate)


def demod(x, baud, carrier, K, samp_rate=96000):
    """(bytes, sync index or -1, o) of one stream."""
    o = acquire(x, baud, carrier, K, samp_rate)[0]
    data, sync = oc.demod(shift(x, o), baud, carrier, K, samp_rate)
    return data, sync, o


def demod_soft(x, baud, carrier, K, samp_rate=96000):
    """(bytes, soft int8, sync index or -1, o) of one stream."""
    o = acquire(x, baud, carrier, K, samp_rate)[0]
    return (*oc.demod_soft(shift(x, o), baud, carrier, K, samp_rate), o)


def delayed(msg: bytes, t: int, baud, carrier, K, tail=None, sigma=0.0, rng=None, samp_rate=96000) -> np.ndarray:
    """A capture of `msg`: t zeros, the frame, `tail` zeros (default L), float32; N(0, sigma^2) on all of it."""
    L = oc.geometry(baud, carrier, K, samp_rate)[1]
    w = oc.modulate(msg, baud, carrier, K, samp_rate)
    x = np.concatenate([np.zeros(t, np.float32), w, np.zeros(L if tail is None else tail, np.float32)])
    if sigma:
        x = x + rng.normal(0.0, sigma, x.size).astype(np.float32)
    return x
