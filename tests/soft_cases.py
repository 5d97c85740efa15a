"""numpy restatement of the soft-decision definitions of DESIGN §3g, the
executable form the host and GPU tests share:

  soft_decode_batch   viterbi_cases.decode_batch with the soft branch metric
                      bm = [c1 != (r1 > 0)] |r1| + [c2 != (r2 > 0)] |r2|
                      (same trellis, tie rule and traceback; -128 reads as
                      -127, 0 is an erasure; both row forms)
  psk_soft            the magnitude rule on the differential products, in
                      float64 in the stated operation order; the products from
                      the oracle's model of numpy's complex multiply, the hard
                      bits from the oracle's slicer
  demod_soft          oracle.psk_symbols -> psk_soft -> sync search, alignment
"""
from __future__ import annotations

import numpy as np

import viterbi_cases as vc
from viterbi_cases import INF, OUT0, P0, P1

MAX_VALS = (1 << 21) - 4
SYNC_BITS = bytes([0, 1, 0, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 1, 0])     # "FB"
_C1, _C2 = (OUT0 >> 1) & 1, OUT0 & 1                                     # the p0 branch's output bits per state


def is_soft_len(n: int) -> bool:
    return 12 <= n <= MAX_VALS and n % 16 in (0, 12)


def bit_stream(row) -> np.ndarray:
    """A soft row of either form as its 16n + 12 coded-bit values (int64), -128 read as -127."""
    v = np.asarray(row, np.int8).astype(np.int64).ravel()
    assert is_soft_len(v.size), v.size
    if v.size % 16 == 0:                                     # the byte image: the last byte's high nibble is skipped
        v = np.concatenate([v[:v.size - 8], v[v.size - 4:]])
    return np.maximum(v, -127)


def byte_image(stream, nibble=0) -> np.ndarray:
    """The byte-aligned form of a bit-stream row: four values `nibble` before the last four."""
    v = np.asarray(stream, np.int8).ravel()
    assert v.size % 16 == 12
    return np.concatenate([v[:-4], np.full(4, nibble, np.int8), v[-4:]])


def from_codeword(cw: bytes, mag: int = 127) -> np.ndarray:
    """The bit-stream row of a hard codeword at +-mag."""
    return ((2 * vc.unpack(cw).astype(np.int16) - 1) * mag).astype(np.int8)


def soft_decode_batch(rows):
    """[(message, metric)] for soft rows of any mix of lengths and forms."""
    vs = [bit_stream(r) for r in rows]
    B = len(vs)
    if B == 0:
        return []
    Ts = np.array([v.size // 2 for v in vs])
    Tm = int(Ts.max())
    r1 = np.zeros((Tm, B), np.int64)                         # steps past a row's own T decide nothing that is read
    r2 = np.zeros((Tm, B), np.int64)
    for i, v in enumerate(vs):
        r1[:Ts[i], i] = v[0::2]
        r2[:Ts[i], i] = v[1::2]
    pm = np.full((B, 64), INF, np.int32)
    pm[:, 0] = 0
    dec = np.zeros((Tm, B, 64), bool)
    metric = np.zeros(B, np.int64)
    ends = {}
    for i, t in enumerate(Ts):
        ends.setdefault(int(t), []).append(i)
    for t in range(Tm):
        a1, a2 = np.abs(r1[t])[:, None], np.abs(r2[t])[:, None]
        h1, h2 = (r1[t] > 0)[:, None], (r2[t] > 0)[:, None]
        bm0 = ((_C1[None, :] != h1) * a1 + (_C2[None, :] != h2) * a2).astype(np.int32)
        bm1 = (a1 + a2).astype(np.int32) - bm0               # the p1 branch's outputs are the complement
        c0 = pm[:, P0] + bm0
        c1 = pm[:, P1] + bm1
        d = c1 < c0                                          # strictly smaller: a tie keeps p0
        pm = np.where(d, c1, c0)
        dec[t] = d
        if t + 1 in ends:
            idx = ends[t + 1]
            metric[idx] = pm[idx, 0]
    s = np.zeros(B, np.int64)
    rows_i = np.arange(B)
    bits = np.zeros((B, Tm), np.uint8)
    for t in range(Tm - 1, -1, -1):
        act = t < Ts
        bits[:, t] = np.where(act, s & 1, 0)
        d = dec[t, rows_i, s]
        s = np.where(act, (s >> 1) | (d.astype(np.int64) << 5), s)
    assert not s.any()
    return [(np.packbits(bits[i, :Ts[i] - 6]).tobytes(), int(metric[i])) for i in range(B)]


def disagreement(row, msg: bytes) -> int:
    """Sum of |r| over the positions where encode(msg)'s bits disagree with the sign of the row."""
    v = bit_stream(row)
    c = vc.encode_bits(msg).astype(bool)
    return int(np.abs(v)[c != (v > 0)].sum())


# ---- PSK soft values -------------------------------------------------------------
def diff_products(sym) -> np.ndarray:
    """s[k+1] * conj(s[k]) as numpy's AVX-512 complex multiply evaluates it (the oracle's model)."""
    from oracle import oracle
    s = np.ascontiguousarray(sym, np.complex128).ravel()
    if s.size < 2:
        return np.zeros(0, np.complex128)
    z, w = np.ascontiguousarray(s[1:]), np.ascontiguousarray(np.conj(s[:-1]))
    ab, mul = np.empty(z.size), np.empty(z.size, np.complex128)
    oracle.lib().oracle_np_complex_model(oracle._p(z), oracle._p(w), z.size, oracle._p(ab), oracle._p(mul))
    return mul


def magnitude(num, den) -> np.ndarray:
    with np.errstate(all="ignore"):
        r = num / den
        q = np.floor(r * 127.0 + 0.5)
    m = np.ones(q.shape, np.int64)
    ok = q >= 1                                              # False for NaN
    m[ok] = np.minimum(q[ok], 127.0).astype(np.int64)
    return m


def psk_soft(kind: str, sym) -> np.ndarray:
    """The soft values of one stream's symbols: int8, 2 (S - 1) (QPSK) or S - 1 (BPSK)."""
    from oracle import oracle
    d = diff_products(sym)
    dr, di = d.real.copy(), d.imag.copy()
    with np.errstate(all="ignore"):
        den = np.abs(dr) + np.abs(di)
        if kind == "bpsk":
            hard = dr < 0
            m = magnitude(np.abs(dr), den)
            return np.where(hard, m, -m).astype(np.int8)
        dib = oracle.qpsk_slice(d)
        mh = magnitude(np.abs(dr + di), den)
        ml = magnitude(np.abs(dr - di), den)
    out = np.empty(2 * d.size, np.int8)
    out[0::2] = np.where(dib & 2, mh, -mh)
    out[1::2] = np.where(dib & 1, ml, -ml)
    return out


def align(soft_all: np.ndarray):
    """(bytes, soft, sync): the sync search over the hard bits and the byte alignment k_sync_pack applies."""
    bits = (soft_all > 0).astype(np.uint8)
    sync = bits.tobytes().find(SYNC_BITS)
    start = max(sync, 0)
    nb = (bits.size - start) // 8
    sl = slice(start, start + 8 * nb)
    return np.packbits(bits[sl]).tobytes(), soft_all[sl].copy(), sync


def demod_soft(kind: str, x, baud, carrier=3000.0, samp_rate=96000, raw_int16=False):
    """(bytes, soft int8, sync index or -1) of one stream."""
    from oracle import oracle
    sym = oracle.psk_symbols(kind, x, baud, carrier, samp_rate, raw_int16=raw_int16)
    if sym.size < 2:
        return b"", np.zeros(0, np.int8), -1
    return align(psk_soft(kind, sym))
