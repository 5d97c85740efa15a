"""numpy restatement of the rate-1/2, K=7 convolutional code (fec.py:79-111,
polynomials 171/133 octal) and of the maximum-likelihood decoder DESIGN §3f
specifies, plus the seeded case generators the host and GPU tests share.

The code
  sr = ((sr << 1) | bit) & 0x7F, message bits MSB-first, then 6 zero bits;
  per step parity(sr & 0x79) then parity(sr & 0x5B); n bytes -> T = 8n + 6
  steps, 16n + 12 coded bits, packed MSB-first into 2n + 2 bytes, the last of
  which holds its 4 bits right-aligned.
The decoder
  state = sr & 0x3F after the step; new state s' has predecessors p0 = s' >> 1
  and p1 = p0 + 32; Hamming branch metrics, int32 path metrics, start 0 at
  state 0 (INF elsewhere), p1 wins only when strictly smaller, traceback over
  the whole codeword from state 0 at step T, decoded bit = bit 0 of the state
  after the step.  metric = the final path metric of state 0.

Everything is vectorised over the 64 states (and over a batch); the only
Python loop is over the steps.
"""
from __future__ import annotations

import numpy as np

G1, G2 = 0x79, 0x5B
INF = 1 << 29
MAX_LEN = 1 << 24

_par = np.array([bin(v).count("1") & 1 for v in range(128)], np.int64)
_S = np.arange(64)
P0 = _S >> 1
P1 = P0 + 32
OUT0 = (_par[_S & G1] << 1) | _par[_S & G2]                # outputs of the p0 branch into state s' (register r0 = s')
_pop2 = np.array([0, 1, 1, 2], np.int64)
BM0 = _pop2[OUT0[None, :] ^ np.arange(4)[:, None]].astype(np.int32)     # [ab][state]
BM1 = (2 - BM0).astype(np.int32)


def is_codeword_len(L: int) -> bool:
    return L % 2 == 0 and 2 <= L <= MAX_LEN


def encode_bits(msg: bytes) -> np.ndarray:
    """The 16n + 12 coded bits of msg (uint8 0/1)."""
    bits = np.concatenate([np.unpackbits(np.frombuffer(bytes(msg), np.uint8)), np.zeros(6, np.uint8)]).astype(np.int64)
    padded = np.concatenate([np.zeros(6, np.int64), bits])
    T = bits.size
    sr = np.zeros(T, np.int64)
    for k in range(7):                                      # register bit k = the input bit k steps ago
        sr |= padded[6 - k:6 - k + T] << k
    out = np.empty(2 * T, np.uint8)
    out[0::2] = _par[sr & G1]
    out[1::2] = _par[sr & G2]
    return out


def codebook_bits(n: int) -> np.ndarray:
    """The coded bits of ALL 256 ** n messages of n bytes, [256 ** n][16n + 12] uint8 (n <= 2):
    row m is message m.to_bytes(n, 'big')."""
    M = 256 ** n
    vals = np.arange(M, dtype=np.int64)
    T = 8 * n + 6
    padded = np.zeros((M, T + 6), np.int64)
    for i in range(8 * n):
        padded[:, 6 + i] = (vals >> (8 * n - 1 - i)) & 1
    sr = np.zeros((M, T), np.int64)
    for k in range(7):
        sr |= padded[:, 6 - k:6 - k + T] << k
    out = np.empty((M, 2 * T), np.uint8)
    out[:, 0::2] = _par[sr & G1]
    out[:, 1::2] = _par[sr & G2]
    return out


def pack(bits: np.ndarray) -> bytes:
    """MSB-first; a last group of fewer than 8 bits stays right-aligned (the reference's loop)."""
    bits = np.asarray(bits, np.uint8)
    full = bits.size // 8 * 8
    out = np.packbits(bits[:full]).tobytes()
    if full < bits.size:
        v = 0
        for b in bits[full:]:
            v = (v << 1) | int(b)
        out += bytes([v])
    return out


def encode(msg: bytes) -> bytes:
    return pack(encode_bits(msg))


def unpack(cw: bytes) -> np.ndarray:
    """The 16n + 12 valid coded bits of a codeword of 2n + 2 bytes (the last byte's low nibble)."""
    a = np.frombuffer(bytes(cw), np.uint8)
    assert is_codeword_len(a.size)
    return np.concatenate([np.unpackbits(a[:-1]), np.unpackbits(a[-1:])[4:]])


def decode_batch(cws):
    """[(message, metric)] for codewords of any mix of lengths, all states and all codewords per numpy call."""
    cws = [bytes(c) for c in cws]
    B = len(cws)
    if B == 0:
        return []
    Ts = np.array([4 * len(c) - 2 for c in cws])
    Tm = int(Ts.max())
    ab = np.zeros((Tm, B), np.int64)                        # steps past a codeword's own T decide nothing that is read
    for i, c in enumerate(cws):
        bits = unpack(c).astype(np.int64)
        ab[:Ts[i], i] = (bits[0::2] << 1) | bits[1::2]
    pm = np.full((B, 64), INF, np.int32)
    pm[:, 0] = 0
    dec = np.zeros((Tm, B, 64), bool)
    metric = np.zeros(B, np.int64)
    ends = {}
    for i, t in enumerate(Ts):
        ends.setdefault(int(t), []).append(i)
    for t in range(Tm):
        a = ab[t]
        c0 = pm[:, P0] + BM0[a]
        c1 = pm[:, P1] + BM1[a]
        d = c1 < c0                                          # strictly smaller: a tie keeps p0
        pm = np.where(d, c1, c0)
        dec[t] = d
        if t + 1 in ends:
            idx = ends[t + 1]
            metric[idx] = pm[idx, 0]
    s = np.zeros(B, np.int64)
    rows = np.arange(B)
    bits = np.zeros((B, Tm), np.uint8)
    for t in range(Tm - 1, -1, -1):
        act = t < Ts
        bits[:, t] = np.where(act, s & 1, 0)
        d = dec[t, rows, s]
        s = np.where(act, (s >> 1) | (d.astype(np.int64) << 5), s)
    assert not s.any()                                       # every path starts in state 0
    return [(np.packbits(bits[i, :Ts[i] - 6]).tobytes(), int(metric[i])) for i in range(B)]


def decode(cw: bytes):
    """(message, metric)."""
    return decode_batch([cw])[0]


def distance(cw: bytes, msg: bytes) -> int:
    """Hamming distance between cw's valid bits and encode(msg)'s."""
    return int(np.count_nonzero(unpack(cw) != encode_bits(msg)))


def flip(cw: bytes, positions) -> bytes:
    """cw with the valid coded bits at `positions` (0 .. 16n + 11) inverted."""
    a = bytearray(cw)
    full = 8 * (len(a) - 1)
    for p in positions:
        p = int(p)
        if p < full:
            a[p // 8] ^= 0x80 >> (p % 8)
        else:
            a[-1] ^= 0x08 >> (p - full)
    return bytes(a)


def set_high_nibble(cw: bytes, nib: int) -> bytes:
    a = bytearray(cw)
    a[-1] = (a[-1] & 0x0F) | ((nib & 0x0F) << 4)
    return bytes(a)


def free_distance(max_depth: int = 1000) -> int:
    """The least weight of a path that leaves state 0 and first returns to it:
    a min-plus recursion over the trellis in which state 0 is not re-entered,
    run until no path still under way is lighter than the best one that returned."""
    w_out = _pop2[OUT0]                                      # weight of the p0 branch into s'
    w_out1 = 2 - w_out                                       # the p1 branch's outputs are the complement
    big = 10 ** 6
    dist = np.full(64, big)
    dist[1] = w_out[1]                                       # 0 -> 1 with input 1 (p0 = 0)
    best = big
    for _ in range(max_depth):
        dist[0] = big                                        # a path that returned has ended
        if dist.min() >= best:
            return best
        cand = np.minimum(dist[P0] + w_out, dist[P1] + w_out1)
        best = min(best, int(cand[0]))
        dist = cand
    raise AssertionError("free distance search did not settle")


def golden():
    """[(kind, message, codeword)] recorded from the reference's encoder (tests/golden/make_conv_golden.py)."""
    import json
    import os
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(g, "conv_manifest.json")) as f:
        man = json.load(f)
    d = np.load(os.path.join(g, "conv.npz"))
    lengths = [int(n) for n in d["lengths"]]
    assert lengths == man["lengths"]
    fills = dict(man["patterns"], rand=None)
    out = []
    for kind, fill in fills.items():
        mo = co = 0
        for n in lengths:
            msg = d["rand_in"][mo:mo + n].tobytes() if fill is None else bytes([fill]) * n
            out.append((kind, msg, d[f"{kind}_out"][co:co + 2 * n + 2].tobytes()))
            mo += n
            co += 2 * n + 2
        assert co == d[f"{kind}_out"].size
    return out


# ---- seeded case generators -----------------------------------------------------
def messages(rng, lengths):
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lengths]


def flip_cases(seed: int, count: int, max_flips: int = 4, max_len: int = 24):
    """(message, received, flips): codewords with 0..max_flips inverted bits and a random high nibble."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(0, max_len + 1))
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        k = int(rng.integers(0, max_flips + 1)) if i >= max_flips + 1 else i      # every count appears
        pos = rng.choice(16 * n + 12, size=k, replace=False)
        rx = set_high_nibble(flip(encode(msg), pos), int(rng.integers(0, 16)))
        out.append((msg, rx, k))
    return out


def noisy(seed: int, lengths, ber: float):
    """(message, received) at a bit-error rate over the valid bits, random high nibble."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        msg = rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()
        nbits = 16 * int(n) + 12
        pos = np.flatnonzero(rng.random(nbits) < ber)
        out.append((msg, set_high_nibble(flip(encode(msg), pos), int(rng.integers(0, 16)))))
    return out


def tie_inputs(seed: int, lengths):
    """Inputs far from every codeword -- dense in metric ties: random bytes, 0x00, 0xFF, 0xAA."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        L = 2 * int(n) + 2
        out += [rng.integers(0, 256, L, dtype=np.uint8).tobytes(), bytes(L), b"\xff" * L, b"\xaa" * L]
    return out
