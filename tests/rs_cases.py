"""The Reed-Solomon code of fec.ReedSolomonCodec restated in numpy -- the
executable specification the host tests establish and the GPU is held bit-equal
to -- and the seeded case generators both test files share.

Field GF(2^8), polynomial 0x11D, alpha = 2; g(x) = prod_{i < nsym} (x - alpha^i);
systematic blocks of k = 255 - nsym message bytes (the last 1 .. k) followed by
nsym parity bytes, first byte the highest power; block interleave as an index
mapping; errors-and-erasures decoding to the unique codeword within
2 e + f <= nsym, or failure."""
from __future__ import annotations

import numpy as np

POLY = 0x11D
N = 255

# ---- the field ------------------------------------------------------------------
EXP = np.zeros(512, np.int64)
LOG = np.zeros(256, np.int64)
_v = 1
for _i in range(255):
    EXP[_i] = _v
    LOG[_v] = _i
    _v <<= 1
    if _v & 0x100:
        _v ^= POLY
EXP[255:510] = EXP[:255]


def mul(a: int, b: int) -> int:
    return int(EXP[LOG[a] + LOG[b]]) if a and b else 0


def inv(a: int) -> int:
    assert a
    return int(EXP[255 - LOG[a]])


def poly_eval(p, x: int) -> int:
    """p ascending: p[0] + p[1] x + ..."""
    r = 0
    for c in reversed(p):
        r = mul(r, x) ^ c
    return r


def generator(nsym: int):
    """g, highest power first: nsym + 1 coefficients, g[0] = 1."""
    g = [1]
    for i in range(nsym):
        root = int(EXP[i])
        g = [a ^ mul(b, root) for a, b in zip(g + [0], [0] + g)]
    return g


# ---- lengths and the interleave ----------------------------------------------------
def encoded_len(n: int, nsym: int) -> int:
    return n + -(-n // (N - nsym)) * nsym


def valid_len(L: int, nsym: int) -> bool:
    if L <= 0:
        return L == 0
    return L - N * (-(-L // N) - 1) >= nsym + 1


def decoded_len(L: int, nsym: int) -> int:
    return L - -(-L // N) * nsym if valid_len(L, nsym) else -1


def block_lens(L: int):
    """The block lengths of a stream of L bytes: 255 each, the last what is left."""
    nblk = -(-L // N)
    return [N] * (nblk - 1) + [L - N * (nblk - 1)] if nblk else []


def stream_index(lens, I: int):
    """For every block the stream positions of its bytes, by emitting the stream:
    groups of I blocks, each column by column, skipping what a short block lacks."""
    idx = [np.zeros(n, np.int64) for n in lens]
    p = 0
    for g0 in range(0, len(lens), I):
        grp = range(g0, min(g0 + I, len(lens)))
        for c in range(N):
            for b in grp:
                if c < lens[b]:
                    idx[b][c] = p
                    p += 1
    return idx


def stream_pos(B: int, c: int, I: int, nblk: int, last_len: int) -> int:
    """The closed form of stream_index (what the kernels compute)."""
    g0 = B // I * I
    b = B - g0
    Ig = min(I, nblk - g0)
    gl = last_len if g0 + Ig == nblk else N
    return g0 * N + (c * Ig + b if c < gl else gl * Ig + (c - gl) * (Ig - 1) + b)


# ---- encode ------------------------------------------------------------------------
def parity(msg: np.ndarray, nsym: int) -> np.ndarray:
    """The remainder of m(x) x^nsym by g: the LFSR, one message byte at a time."""
    g = generator(nsym)[1:]
    lg = [int(LOG[c]) for c in g]                          # no coefficient of g is 0 below degree 255
    reg = [0] * nsym
    for m in msg:
        fb = int(m) ^ reg[0]
        reg = reg[1:] + [0]
        if fb:
            lf = int(LOG[fb])
            reg = [r ^ int(EXP[lf + l]) for r, l in zip(reg, lg)]
    return np.array(reg, np.uint8)


def encode_blocks(msg: bytes, nsym: int):
    a = np.frombuffer(bytes(msg), np.uint8)
    k = N - nsym
    return [np.concatenate([a[i:i + k], parity(a[i:i + k], nsym)]) for i in range(0, a.size, k)]


def encode(msg: bytes, nsym: int = 32, I: int = 1) -> bytes:
    blocks = encode_blocks(msg, nsym)
    out = np.zeros(sum(b.size for b in blocks), np.uint8)
    for b, ix in zip(blocks, stream_index([b.size for b in blocks], I)):
        out[ix] = b
    return out.tobytes()


# ---- decode ----------------------------------------------------------------------
def syndromes(r: np.ndarray, nsym: int) -> np.ndarray:
    """S_j = r(alpha^j) = sum_c r_c alpha^(j (len - 1 - c)), j < nsym."""
    n = r.size
    nz = np.nonzero(r)[0]
    if nz.size == 0:
        return np.zeros(nsym, np.int64)
    e = (LOG[r[nz]][None, :] + np.arange(nsym)[:, None] * (n - 1 - nz)[None, :]) % 255
    return np.bitwise_xor.reduce(EXP[e], axis=1)


def decode_block(rx: np.ndarray, erased: np.ndarray, nsym: int):
    """(codeword, corrected) or (None, 0): the unique codeword that differs from rx
    in e positions outside `erased` with 2 e + f <= nsym, by Berlekamp-Massey from
    the erasure locator, Chien, Forney -- and then CHECKED against that definition,
    so a wrong step can only turn into a failure the brute-force tests catch."""
    n = rx.size
    f = int(erased.sum())
    if f > nsym:
        return None, 0
    r = rx.copy()
    r[erased] = 0
    S = [int(s) for s in syndromes(r, nsym)]
    X = [int(EXP[(n - 1 - c) % 255]) for c in range(n)]
    lam = [1]
    for c in np.nonzero(erased)[0]:                        # the erasure locator prod (1 - X x)
        lam = [a ^ mul(b, X[c]) for a, b in zip(lam + [0], [0] + lam)]
    B, L, m, b = list(lam), f, 1, 1
    for i in range(f, nsym):
        delta = 0
        for j in range(min(L, len(lam) - 1) + 1):
            delta ^= mul(lam[j], S[i - j])
        if delta == 0:
            m += 1
            continue
        scale = mul(delta, inv(b))
        shifted = [0] * m + [mul(scale, c) for c in B]
        nxt = [(lam[j] if j < len(lam) else 0) ^ (shifted[j] if j < len(shifted) else 0)
               for j in range(max(len(lam), len(shifted)))]
        if 2 * L <= i + f:
            B, b, L, m = list(lam), delta, i + 1 - L + f, 1
        else:
            m += 1
        lam = nxt
    if 2 * L > nsym + f:
        return None, 0
    lam = (lam + [0] * (L + 1))[:L + 1]
    roots = [c for c in range(n) if poly_eval(lam, inv(X[c])) == 0]
    if len(roots) != L:
        return None, 0
    omega = [0] * nsym
    for i in range(nsym):
        for j in range(min(i, L) + 1):
            omega[i] ^= mul(lam[j], S[i - j])
    deriv = [lam[j] if j % 2 else 0 for j in range(1, L + 1)]      # d/dx: the odd coefficients, one power down
    for c in roots:
        xi = inv(X[c])
        den = poly_eval(deriv, xi)
        if den == 0:
            return None, 0
        r[c] ^= mul(mul(X[c], poly_eval(omega, xi)), inv(den))
    if syndromes(r, nsym).any():
        return None, 0
    e = int(np.count_nonzero((r != rx) & ~erased))
    if 2 * e + f > nsym:
        return None, 0
    return r, int(np.count_nonzero(r != rx))


def decode(data: bytes, nsym: int = 32, I: int = 1, erase_pos=None):
    """(message, corrected, failed); failed = -1 and an empty message for an invalid length."""
    a = np.frombuffer(bytes(data), np.uint8)
    if not valid_len(a.size, nsym):
        return b"", 0, -1
    er = np.zeros(a.size, bool)
    if erase_pos is not None and len(erase_pos):
        er[np.asarray(list(erase_pos), np.int64)] = True
    lens = block_lens(a.size)
    out, corrected, failed = [], 0, 0
    for n, ix in zip(lens, stream_index(lens, I)):
        rx = a[ix]
        cw, nfix = decode_block(rx, er[ix], nsym)
        if cw is None:
            failed += 1
            cw = rx
        corrected += nfix
        out.append(cw[:n - nsym])
    return (np.concatenate(out).tobytes() if out else b""), corrected, failed


def decode_batch(datas, nsym=32, I=1, erasures=None):
    return [decode(d, nsym, I, None if erasures is None else erasures[i]) for i, d in enumerate(datas)]


# ---- brute force (independent of everything above but the field and the encoder) ------
def pattern_syndromes(n: int, nsym: int, weight: int):
    """Every error pattern of weight <= `weight` (1 or 2) on a block of n bytes:
    (keys, positions [m][2], values [m][2]) with keys the syndromes packed into
    one integer, sorted.  The syndrome is linear, so rx + pattern is a codeword
    exactly when the pattern's syndromes equal rx's."""
    j = np.arange(nsym)
    shifts = 8 * j
    def synd(pos, val):                                      # pos, val [m]
        e = (LOG[val][:, None] + j[None, :] * (n - 1 - pos)[:, None]) % 255
        return EXP[e]
    keys, poss, vals = [np.zeros(1, np.int64)], [np.full((1, 2), -1)], [np.zeros((1, 2), np.int64)]
    p1, v1 = np.meshgrid(np.arange(n), np.arange(1, 256), indexing="ij")
    p1, v1 = p1.ravel(), v1.ravel()
    s1 = synd(p1, v1)
    keys.append((s1 << shifts).sum(axis=1))
    poss.append(np.stack([p1, np.full_like(p1, -1)], axis=1))
    vals.append(np.stack([v1, np.zeros_like(v1)], axis=1))
    if weight >= 2:
        for a in range(n):
            for b in range(a + 1, n):
                va, vb = np.meshgrid(np.arange(1, 256), np.arange(1, 256), indexing="ij")
                va, vb = va.ravel(), vb.ravel()
                s2 = synd(np.full_like(va, a), va) ^ synd(np.full_like(vb, b), vb)
                keys.append((s2 << shifts).sum(axis=1))
                poss.append(np.stack([np.full_like(va, a), np.full_like(vb, b)], axis=1))
                vals.append(np.stack([va, vb], axis=1))
    keys = np.concatenate(keys)
    poss = np.concatenate([p.astype(np.int8) for p in poss])
    vals = np.concatenate([v.astype(np.uint8) for v in vals])
    order = np.argsort(keys, kind="stable")
    return keys[order], poss[order], vals[order]


def brute_errors(rx: np.ndarray, nsym: int, table):
    """The codeword within floor(nsym / 2) errors of rx by the pattern table, or None.
    More than one pattern with rx's syndromes would contradict the distance: asserted."""
    keys, poss, vals = table
    key = int((syndromes(rx, nsym) << (8 * np.arange(nsym))).sum())
    lo, hi = np.searchsorted(keys, key, "left"), np.searchsorted(keys, key, "right")
    assert hi - lo <= 1
    if hi == lo:
        return None
    cw = rx.copy()
    for p, v in zip(poss[lo], vals[lo]):
        if p >= 0:
            cw[p] ^= v
    return cw


def codebook(n: int, nsym: int) -> np.ndarray:
    """Every codeword of length n (n - nsym <= 2 message bytes): [256^(n-nsym)][n]."""
    kk = n - nsym
    assert 1 <= kk <= 2
    msgs = np.stack(np.meshgrid(*[np.arange(256)] * kk, indexing="ij"), axis=-1).reshape(-1, kk)
    g = generator(nsym)[1:]
    mt = np.array([[mul(a, b) for b in range(256)] for a in g], np.int64)     # [nsym][256]: g_j * v
    reg = np.zeros((msgs.shape[0], nsym), np.int64)
    for c in range(kk):
        fb = msgs[:, c] ^ reg[:, 0]
        reg = np.concatenate([reg[:, 1:], np.zeros((msgs.shape[0], 1), np.int64)], axis=1) ^ mt[:, fb].T
    return np.concatenate([msgs, reg], axis=1).astype(np.uint8)


def brute_codebook(rx: np.ndarray, erased: np.ndarray, nsym: int, book: np.ndarray):
    """The codewords c with 2 e + f <= nsym (e = the positions outside `erased` where c differs from rx)."""
    f = int(erased.sum())
    e = np.count_nonzero(book[:, ~erased] != rx[None, ~erased], axis=1)
    return book[2 * e + f <= nsym]


# ---- seeded cases ------------------------------------------------------------------
def messages(rng, lengths):
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lengths]


def msg_len_for_last_block(nblk: int, last_cw_len: int, nsym: int) -> int:
    """The message length whose encoding has nblk blocks, the last a codeword of last_cw_len bytes."""
    assert nsym + 1 <= last_cw_len <= N
    return (nblk - 1) * (N - nsym) + last_cw_len - nsym


def corrupt_blocks(rng, cw: bytes, nsym: int, I: int, n_err, where="any", n_erase=0, erase_right=0):
    """Corrupt every block of the encoded stream cw: n_err wrong bytes per block
    (where: "any", "parity", "ends" = the block's first and last byte first) and
    n_erase erased positions, disjoint from the errors; erased bytes get random
    values except the first erase_right of them, which stay correct.
    Returns (received bytes, erased stream positions)."""
    a = np.frombuffer(cw, np.uint8).copy()
    lens = block_lens(a.size)
    erased = []
    for n, ix in zip(lens, stream_index(lens, I)):
        ne = min(int(n_err), n)
        if where == "parity":
            pool = np.arange(n - nsym, n)
            ne = min(ne, nsym)
        else:
            pool = np.arange(n)
        if where == "ends" and ne >= 2:
            pos = np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), ne - 2, replace=False)])
        else:
            pos = rng.choice(pool, ne, replace=False)
        a[ix[pos]] ^= rng.integers(1, 256, ne, dtype=np.uint8)
        free = np.setdiff1d(np.arange(n), pos)
        nz = min(int(n_erase), free.size)
        ep = rng.choice(free, nz, replace=False)
        for t, c in enumerate(ep):
            if t >= erase_right:
                a[ix[c]] = rng.integers(0, 256)
        erased += [int(ix[c]) for c in ep]
    return a.tobytes(), sorted(erased)


def chain_case(seed: int, ber: float, n_msgs: int = 4, n_bytes: int = 446, nsym: int = 32, I: int = 2):
    """The concatenated code: messages -> RS (outer) -> K=7 convolutional (inner),
    then coded bits inverted at rate `ber`.  Returns (messages, outer codewords, received inner codewords)."""
    import viterbi_cases as vc
    rng = np.random.default_rng(seed)
    msgs = messages(rng, [n_bytes] * n_msgs)
    outer = [encode(m, nsym, I) for m in msgs]
    rx = []
    for o in outer:
        pos = np.flatnonzero(rng.random(16 * len(o) + 12) < ber)
        rx.append(vc.flip(vc.encode(o), pos))
    return msgs, outer, rx
