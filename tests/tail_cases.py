"""The integer tail of the receiver -- sync search + byte pack (k_sync_pack),
parity-triple FEC decode (k_fec_decode), FBP frame parse (k_frame_parse) --
restated plainly, with the seeded case families its tests share.  No GPU, no
oracle: str.find / int(.., 2), zlib.crc32, bytes.find / struct.unpack /
binascii.crc32.

The restatements are written from the behaviour, and pinned to the reference
itself: tests/golden/make_tail_golden.py runs the reference on every case
below and keeps one SHA-256 per family (tail_digests.json); test_tail_cases.py
recomputes the digests from the restatements here.  test_gpu_tail.py then
holds the kernels to the restatements, case by case.
"""
from __future__ import annotations

import binascii
import hashlib
import json
import struct
import zlib

import numpy as np

SYNC = "0100011001000010"                 # "FB", the first 16 bits of the frame magic
SYNC_BITS = np.array([int(c) for c in SYNC], np.uint8)

# k_frame_parse's per-candidate verdicts (include/amr.h AMR_FRAME_*)
SHORT, NONAME, NOMETA, BADLEN, INCOMPLETE, CRC_BAD, OK = range(7)
REC_FIELDS = ("start", "name_start", "name_len", "payload_start", "part", "total", "fsize", "fcrc", "dlen", "pcrc",
              "status")


# ---------------------------------------------------------------------------
# plain restatements
def bit_string(bits) -> str:
    return (np.asarray(bits, np.uint8) + 48).tobytes().decode("ascii")


def ref_sync_pack(bits):
    """(bytes, sync index or -1): the whole bytes of the bit string from its
    first SYNC, or from bit 0 when there is none."""
    s = bit_string(bits)
    idx = s.find(SYNC)
    body = s[idx:] if idx >= 0 else s
    return bytes(int(body[i:i + 8], 2) for i in range(0, len(body) - 7, 8)), idx


def ref_fec_decode(data: bytes):
    """(decoded, crc_ok).  Under 4 bytes: unchanged, ok.  Else the last 4 bytes
    are a little-endian CRC32 of the decoded bytes; the body is (b1, b2, parity)
    triples giving b1, b2 -- or b1, '?' when b1 ^ b2 != parity -- and a tail of
    one or two bytes that is copied."""
    data = bytes(data)
    if len(data) < 4:
        return data, True
    body, want = data[:-4], int.from_bytes(data[-4:], "little")
    full = len(body) // 3
    out = bytearray()
    for t in range(full):
        b1, b2, par = body[3 * t], body[3 * t + 1], body[3 * t + 2]
        out.append(b1)
        out.append(b2 if b1 ^ b2 == par else 0x3F)
    out += body[3 * full:]
    return bytes(out), zlib.crc32(out) == want


def ref_frame_parse(raw: bytes):
    """(records, frames, log) of one decoded stream.  records: one dict per
    b'FBPC' occurrence, in order, with the check that stopped it (or the CRC
    verdict) as `status`; a header field the parse never reached is 0, and
    `calc_crc` is there for OK / CRC_BAD only.  frames: the accepted
    {'name', 'data', 'final_crc'}.  log: the lines the parser prints."""
    raw = bytes(raw)
    L = len(raw)
    starts, at = [], raw.find(b"FBPC")
    while at >= 0:
        starts.append(at)
        at = raw.find(b"FBPC", at + 1)
    log = [f"Encontrados {len(starts)} candidatos a cabeçalho."]
    records, frames = [], []
    for start in starts:
        r = dict.fromkeys(REC_FIELDS, 0)
        r["start"] = start
        records.append(r)
        if L - start < 30:
            r["status"] = SHORT
            continue
        r["name_len"], r["name_start"] = raw[start + 4], start + 5
        if r["name_len"] == 0:
            r["status"] = NONAME
            continue
        meta = r["name_start"] + r["name_len"]
        if L - meta < 24:
            r["status"] = NOMETA
            continue
        r["part"], r["total"], r["fsize"], r["fcrc"], r["dlen"], r["pcrc"] = struct.unpack("<6I", raw[meta:meta + 24])
        r["payload_start"] = meta + 24
        if not 1 <= r["dlen"] <= 50_000_000:
            r["status"] = BADLEN
            continue
        name = raw[r["name_start"]:meta].decode("utf-8", "ignore")
        if L - r["payload_start"] < r["dlen"]:
            r["status"] = INCOMPLETE
            log.append(f"Dados incompletos para {name}")
            continue
        payload = raw[r["payload_start"]:r["payload_start"] + r["dlen"]]
        r["calc_crc"] = binascii.crc32(payload) & 0xFFFFFFFF
        if r["calc_crc"] == r["pcrc"]:
            r["status"] = OK
            log.append(f"✅ CRC VÁLIDO: {name} (Parte {r['part'] + 1}/{r['total']})")
            frames.append({"name": name, "data": payload, "final_crc": r["fcrc"]})
        else:
            r["status"] = CRC_BAD
            log.append(f"❌ Erro de CRC para {name}")
    return records, frames, "".join(line + "\n" for line in log)


# ---------------------------------------------------------------------------
# digests (what tests/golden/tail_digests.json holds per family)
def sync_result_blob(out: bytes, idx: int) -> bytes:
    return struct.pack("<q", len(out)) + out + struct.pack("<q", idx)


def fec_result_blob(out: bytes, warned: bool) -> bytes:
    return struct.pack("<q", len(out)) + out + bytes([1 if warned else 0])


def frame_result_blob(frames, log: str) -> bytes:
    doc = json.dumps({"frames": [{"name": f["name"], "data": bytes(f["data"]).hex(), "final_crc": int(f["final_crc"])}
                                 for f in frames], "log": log}, ensure_ascii=True, sort_keys=True).encode()
    return struct.pack("<q", len(doc)) + doc


def digest(blobs) -> dict:
    h = hashlib.sha256()
    n = 0
    for b in blobs:
        h.update(b)
        n += 1
    return {"cases": n, "sha256": h.hexdigest()}


# ---------------------------------------------------------------------------
# sync / pack cases.  A case is (label, row, n_bits, n_words): row holds the
# n_bits valid bits and then, where the case is about them, stale bits up to
# n_words * 32 that nothing may read.  n_words None: ceil(n_bits / 32), at least 1.
def _plant(row, p):
    row[p:p + 16] = SYNC_BITS
    return row


def _filler(rng, n, kind):
    return np.zeros(n, np.uint8) if kind == "zero" else rng.integers(0, 2, n, dtype=np.uint8)


def sync_sweep_cases():
    """n_bits 0..160 x a sync at every p in 0..n_bits-16 (and one row without a
    planted sync), over a zero and a seeded random filler."""
    rng = np.random.default_rng(4201)
    cases = []
    for kind in ("zero", "rand"):
        for n in range(161):
            cases.append((f"sweep/{kind}/n{n}/none", _filler(rng, n, kind), n, None))
            for p in range(n - 15):
                cases.append((f"sweep/{kind}/n{n}/p{p}", _plant(_filler(rng, n, kind), p), n, None))
    return cases


def sync_cut_cases():
    """The pattern starts at n_bits - 15: its last bit is missing.  Everything
    past n_bits -- the rest of the last word, and three further words in the
    second variant -- repeats the pattern, so reading any of it completes one."""
    cases = []
    for extra in (0, 3):
        for n in range(161):
            nw = max(1, (n + 31) // 32) + extra
            start = max(0, n - 15)
            row = np.zeros(nw * 32, np.uint8)
            reps = (nw * 32 - start + 15) // 16
            row[start:] = np.tile(SYNC_BITS, reps)[:nw * 32 - start]
            cases.append((f"cut/x{extra}/n{n}", row, n, nw))
    return cases


LONG_N = (2048, 2049, 4096 + 17, 6200)


def sync_long_cases():
    """Rows longer than one 64-word search pass: one sync at every p around the
    pass boundaries (bits 2048 and 4096), at the last legal p, and none."""
    rng = np.random.default_rng(4202)
    cases = []
    for kind in ("zero", "rand"):
        for n in LONG_N:
            ps = [p for c in (2048, 4096) for p in range(c - 40, c + 41) if p + 16 <= n]
            for p in sorted(set(ps + [n - 16])):
                cases.append((f"long/{kind}/n{n}/p{p}", _plant(_filler(rng, n, kind), p), n, None))
            cases.append((f"long/{kind}/n{n}/none", _filler(rng, n, kind), n, None))
    return cases


TWO_N = 6200
TWO_PAIRS = [
    ("same_word", 32 * 5, 32 * 5 + 16), ("same_word_hi", 32 * 70 + 3, 32 * 70 + 19),
    ("adjacent", 32 * 9 + 5, 32 * 10 + 9), ("adjacent_overlap", 32 * 9 + 20, 32 * 10 + 4),
    ("adjacent_pass_edge", 32 * 63 + 1, 32 * 64 + 2), ("lane63_lane0", 32 * 63 + 30, 32 * 64 + 20),
    ("late_early", 32 * 60 + 7, 32 * 66 + 11), ("mid_early", 32 * 40, 32 * 67 + 31),
    ("pass0_pass2", 32 * 10 + 13, 32 * 130 + 2), ("pass1_pass2", 32 * 100 + 9, 32 * 129 + 17),
    ("pass1_pass3", 32 * 127 + 31, 32 * 192 + 0),
]


def sync_two_cases():
    """Two syncs in zeros: the first must win, whichever lane or pass finds the other."""
    cases = []
    for label, p1, p2 in TWO_PAIRS:
        row = _plant(_plant(np.zeros(TWO_N, np.uint8), p2), p1)
        cases.append((f"two/{label}", row, TWO_N, None))
    return cases


PACK_NBYTES = list(range(10)) + list(range(253, 261)) + list(range(509, 517))


def sync_pack_cases():
    """Packed byte counts 0..9, 253..260, 509..516 (the packer writes 256 bytes a
    pass, 4 a lane): from a sync at bit s, and from bit 0 without one, with 0, 3
    or 7 bits left over."""
    rng = np.random.default_rng(4203)
    cases = []
    for nbytes in PACK_NBYTES:
        for left in (0, 3, 7):
            n = 8 * nbytes + left
            row = rng.integers(0, 2, n, dtype=np.uint8)
            while (at := bit_string(row).find(SYNC)) >= 0:  # no sync anywhere: packed from bit 0
                row[at + 1] = 0
            cases.append((f"pack/b{nbytes}/left{left}/nosync", row, n, None))
            if nbytes < 2:
                continue
            for s in (0, 5, 31, 37):
                n = s + 8 * nbytes + left
                row = rng.integers(0, 2, n, dtype=np.uint8)
                row[:s] = 0
                cases.append((f"pack/b{nbytes}/left{left}/s{s}", _plant(row, s), n, None))
    return cases


def sync_random_cases():
    """4096 rows: 64 seeded lengths up to 3000 bits, 64 random rows each, every
    other one with a sync planted at a random place."""
    rng = np.random.default_rng(4204)
    cases = []
    for n in sorted(int(v) for v in rng.integers(0, 3001, 64)):
        for k in range(64):
            row = rng.integers(0, 2, n, dtype=np.uint8)
            if k % 2 and n >= 16:
                _plant(row, int(rng.integers(0, n - 15)))
            cases.append((f"random/n{n}/{k}", row, n, None))
    return cases


COMPANION_PSK_BAUD = 1000                 # QPSK round-trips there (test_gpu_loopback.py)
COMPANION_FSK = (1200, 2400.0, 4800.0)    # baud, mark, space: likewise


def companion_payloads(n_bytes: int = 24):
    """64 payloads of n_bytes for the real demodulators: payload k is k zero
    bits, the 16 sync bits, then seeded data up to n_bytes whole bytes."""
    rng = np.random.default_rng(4205)
    out = []
    for k in range(64):
        bits = np.concatenate([np.zeros(k, np.uint8), SYNC_BITS, rng.integers(0, 2, 8 * n_bytes - 16 - k, dtype=np.uint8)])
        out.append(np.packbits(bits).tobytes())
    return out


SYNC_FAMILIES = {"sync_sweep": sync_sweep_cases, "sync_cut": sync_cut_cases, "sync_long": sync_long_cases,
                 "sync_two": sync_two_cases, "sync_pack": sync_pack_cases, "sync_random": sync_random_cases}


# ---------------------------------------------------------------------------
# FEC cases: (label, encoded bytes) per variant, over every input length
FEC_LENGTHS = list(range(801)) + [4099, 65_541, 200_003]


def _fec_encode(decoded: bytes, rem: int) -> bytearray:
    """The body whose decode is `decoded`: consistent triples, then `rem` tail bytes."""
    nt = (len(decoded) - rem) // 2
    d = np.frombuffer(decoded, np.uint8)
    body = np.empty(3 * nt + rem, np.uint8)
    body[0:3 * nt:3] = d[0:2 * nt:2]
    body[1:3 * nt:3] = d[1:2 * nt:2]
    body[2:3 * nt:3] = d[0:2 * nt:2] ^ d[1:2 * nt:2]
    body[3 * nt:] = d[2 * nt:]
    return bytearray(body.tobytes())


def _crc_le(decoded: bytes) -> bytes:
    return struct.pack("<I", zlib.crc32(decoded) & 0xFFFFFFFF)


def fec_cases(variant: str):
    """variant: 'valid' (consistent parities, correct CRC); 'broken_first' /
    'broken_last' / 'broken_seeded' (one triple's parity broken, the CRC over
    the decoded bytes with its '?'); 'crc_flip' (valid, one CRC bit flipped);
    'byte_flip' (valid, the last decoded byte changed); 'random'."""
    rng = np.random.default_rng(4300 + sorted(FEC_VARIANTS).index(variant))
    cases = []
    for n in FEC_LENGTHS:
        if n < 4 or variant == "random":
            cases.append((f"{variant}/n{n}", rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
            continue
        nt, rem = divmod(n - 4, 3)
        decoded = bytearray(rng.integers(0, 256, 2 * nt + rem, dtype=np.uint8).tobytes())
        body = _fec_encode(bytes(decoded), rem)
        crc = bytearray(_crc_le(bytes(decoded)))
        if variant.startswith("broken"):
            if nt == 0:
                continue                                    # no triple to break
            t = {"broken_first": 0, "broken_last": nt - 1}.get(variant, int(rng.integers(0, nt)))
            body[3 * t + 2] ^= int(rng.integers(1, 256))
            decoded[2 * t + 1] = 0x3F
            crc = bytearray(_crc_le(bytes(decoded)))
        elif variant == "crc_flip":
            crc[int(rng.integers(0, 4))] ^= 1 << int(rng.integers(0, 8))
        elif variant == "byte_flip":
            if not decoded:
                continue                                    # nothing decoded to change
            mask = 1 << int(rng.integers(0, 8))
            if rem:
                body[-1] ^= mask                            # the copied tail's last byte
            else:
                body[-2] ^= mask                            # b2 and its parity together:
                body[-1] ^= mask                            # still consistent, another byte
        cases.append((f"{variant}/n{n}", bytes(body) + bytes(crc)))
    return cases


FEC_VARIANTS = ("valid", "broken_first", "broken_last", "broken_seeded", "crc_flip", "byte_flip", "random")


# ---------------------------------------------------------------------------
# frame cases: (label, stream)
def frame(name: bytes, payload: bytes, part=0, total=1, fcrc=0x1234) -> bytes:
    meta = struct.pack("<6I", part, total, len(payload), fcrc, len(payload), binascii.crc32(payload) & 0xFFFFFFFF)
    return b"FBPC" + bytes([len(name)]) + name + meta + payload


def filler(rng, n: int) -> bytes:
    """n seeded bytes with no 'F' among them: no magic, whatever follows."""
    a = rng.integers(0, 256, n, dtype=np.uint8)
    a[a == 0x46] = 0x47
    return a.tobytes()


def _name(rng, n: int) -> bytes:
    return bytes(rng.integers(0x61, 0x7B, n, dtype=np.uint8))          # a..z: no magic, no 'F'


FIT_PAYLOADS = list(range(1, 201)) + [255, 256, 257, 4095, 4096, 4097, 65_537]


def frame_fit_cases():
    """One frame, the stream ending exactly at its payload's end, one byte short
    of it and one byte past it; each also with the last payload byte changed."""
    rng = np.random.default_rng(4401)
    cases = []
    for nl in (1, 2, 255):
        for dl in FIT_PAYLOADS:
            fr = frame(_name(rng, nl), filler(rng, dl), part=int(rng.integers(0, 9)), total=9,
                       fcrc=int(rng.integers(0, 1 << 32)))
            bad = fr[:-1] + bytes([fr[-1] ^ 0x10])
            for tag, f in (("good", fr), ("flip", bad)):
                cases.append((f"fit/nl{nl}/d{dl}/{tag}/exact", f))
                cases.append((f"fit/nl{nl}/d{dl}/{tag}/short", f[:-1]))
                cases.append((f"fit/nl{nl}/d{dl}/{tag}/long", f + b"\x00"))
    return cases


def frame_header_cases():
    """Streams cut at the two header checks: start + 29 / 30 / 31 bytes, and
    meta_start + 23 / 24 / 25 bytes (a one-byte payload: the last is whole)."""
    rng = np.random.default_rng(4402)
    cases = []
    for start in (0, 13, 61):
        fr = filler(rng, start) + frame(b"n", b"\x07")                 # 31 bytes from its magic
        for cut in (29, 30, 31):
            cases.append((f"header/start{start}/+{cut}", fr[:start + cut]))
        for nl in (2, 100, 255):
            fr = filler(rng, start) + frame(_name(rng, nl), b"\x09")
            meta = start + 5 + nl
            for cut in (23, 24, 25):
                cases.append((f"header/start{start}/nl{nl}/meta+{cut}", fr[:meta + cut]))
    return cases


def frame_scan_cases():
    """The scan's 64-byte blocks: a valid frame starting at every offset 56..70
    behind magic-free filler (also behind a broken-off 'FBP'), and a bare magic
    ending exactly at L for L in 4..140."""
    rng = np.random.default_rng(4403)
    cases = []
    for off in range(56, 71):
        fr = frame(b"s.bin", filler(rng, 40))
        cases.append((f"scan/frame@{off}", filler(rng, off) + fr + filler(rng, 9)))
        cases.append((f"scan/frame@{off}/after_FBP", filler(rng, off - 3) + b"FBP" + fr))
    for L in range(4, 141):
        cases.append((f"scan/magic_ends@{L}", filler(rng, L - 4) + b"FBPC"))
    return cases


CAPS = (1, 2, 63, 64, 65, 255, 256)


def frame_cap_cases(max_cands: int):
    """Streams of exactly max_cands - 1, max_cands and max_cands + 1 short valid frames."""
    rng = np.random.default_rng(4404 + max_cands)
    cases = []
    for count in (max_cands - 1, max_cands, max_cands + 1):
        body = b"".join(frame(_name(rng, 1 + k % 3), filler(rng, 1 + k % 5), part=k, total=count) + filler(rng, k % 4)
                        for k in range(count))
        cases.append((f"cap{max_cands}/count{count}", body))
    return cases


def frame_families():
    fam = {"frame_fit": frame_fit_cases(), "frame_header": frame_header_cases(), "frame_scan": frame_scan_cases()}
    fam["frame_caps"] = [c for mc in CAPS for c in frame_cap_cases(mc)]
    return fam


# ---------------------------------------------------------------------------
def restated_digests() -> dict:
    """Every family's digest, from the restatements above."""
    out = {}
    for fam, gen in SYNC_FAMILIES.items():
        out[fam] = digest(sync_result_blob(*ref_sync_pack(row[:n])) for _, row, n, _ in gen())
    for v in FEC_VARIANTS:
        res = ((d, ref_fec_decode(d)) for _, d in fec_cases(v))
        out["fec_" + v] = digest(fec_result_blob(o, len(d) >= 4 and not ok) for d, (o, ok) in res)
    for fam, cases in frame_families().items():
        out[fam] = digest(frame_result_blob(*ref_frame_parse(raw)[1:]) for _, raw in cases)
    return out
