"""tests/tail_cases.py without a GPU: its plain restatements give, on every
seeded case, exactly what the REFERENCE gave (one SHA-256 per family in
tests/golden/tail_digests.json, written by make_tail_golden.py), and the case
families hold what their names promise -- the conditions test_gpu_tail.py
relies on when it compares the kernels with the restatements."""
import json
import os

import pytest

import tail_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def restated():
    return tc.restated_digests()


def test_restatements_match_the_reference_digests(restated):
    with open(os.path.join(HERE, "golden", "tail_digests.json")) as f:
        want = json.load(f)["families"]
    assert sorted(restated) == sorted(want)
    for fam in sorted(want):
        assert restated[fam] == want[fam], fam


def test_sync_families_hold_their_conditions():
    sweep = tc.sync_sweep_cases()
    assert len(sweep) == 2 * (161 + sum(n - 15 for n in range(16, 161)))
    for label, row, n, _ in sweep:
        if "/zero/" in label and "/p" in label:
            assert tc.ref_sync_pack(row)[1] == int(label.rsplit("/p", 1)[1]), label
    for label, row, n, nw in tc.sync_cut_cases():
        assert tc.ref_sync_pack(row[:n])[1] == -1, label                    # cut: no sync in the valid bits ...
        assert row.size == nw * 32
        if row.size > n:                         # ... the stale ones complete it (n % 32 == 0: a zero past the row would)
            assert tc.ref_sync_pack(row[:max(n + 1, 16)])[1] == max(0, n - 15), label
    for label, row, n, _ in tc.sync_long_cases():
        if "/zero/" in label:
            want = -1 if label.endswith("none") else int(label.rsplit("/p", 1)[1])
            assert tc.ref_sync_pack(row)[1] == want, label
    assert {n for _, _, n, _ in tc.sync_long_cases()} == set(tc.LONG_N)
    for (label, row, n, _), (_, p1, p2) in zip(tc.sync_two_cases(), tc.TWO_PAIRS):
        assert p1 < p2 and tc.ref_sync_pack(row)[1] == p1, label
        assert tc.bit_string(row).find(tc.SYNC, p1 + 1) == p2, label
    seen = set()
    for label, row, n, _ in tc.sync_pack_cases():
        out, idx = tc.ref_sync_pack(row)
        assert idx == (-1 if label.endswith("nosync") else int(label.rsplit("/s", 1)[1])), label
        seen.add(len(out))
    assert seen == set(tc.PACK_NBYTES)
    rnd = tc.sync_random_cases()
    assert len(rnd) == 4096 and max(n for _, _, n, _ in rnd) <= 3000
    assert sum(tc.ref_sync_pack(row)[1] >= 0 for _, row, _, _ in rnd) >= 2000


def test_companion_streams_give_consecutive_syncs_in_the_oracle():
    """The 64 payloads whose sync sits k = 0..63 bits in: through the oracle's
    own modulators and demodulators the sync indices are 64 consecutive values,
    so test_gpu_tail.py may ask the same of the GPU."""
    import numpy as np
    from oracle import oracle
    pays = tc.companion_payloads()
    assert len(pays) == 64 and {len(p) for p in pays} == {24}
    for k, p in enumerate(pays):
        assert tc.ref_sync_pack(np.unpackbits(np.frombuffer(p, np.uint8)))[1] == k
    x = np.stack([oracle.qpsk_modulate(p, baud=tc.COMPANION_PSK_BAUD) for p in pays])
    outs, sync = oracle.psk_demod_batch("qpsk", x, tc.COMPANION_PSK_BAUD)
    assert [int(s) - int(sync[0]) for s in sync] == list(range(64)), list(sync)
    assert all(outs[k].startswith(pays[k][k // 8:]) for k in range(0, 64, 8))      # the planted sync is the one found
    baud, mark, space = tc.COMPANION_FSK
    res = [oracle.fsk_demodulate(oracle.fsk_modulate(p, baud, mark, space), baud, mark, space, return_sync=True)
           for p in pays]
    assert [r[1] - res[0][1] for r in res] == list(range(64)), [r[1] for r in res]
    assert res[0][0].startswith(pays[0])


def test_fec_variants_hold_their_conditions():
    lens = lambda v: [len(d) for _, d in tc.fec_cases(v)]   # noqa: E731
    assert lens("valid") == tc.FEC_LENGTHS == lens("random") == lens("crc_flip")
    decoded_lens = {(n - 4) // 3 * 2 + (n - 4) % 3 for n in tc.FEC_LENGTHS if n >= 4}
    assert {(n - 4) % 3 for n in range(4, 801)} == {0, 1, 2}
    for k in range(1, 9):                                    # the decoded length steps across 64 k, k up to 8
        for d in (64 * k - 1, 64 * k, 64 * k + 1):
            assert d in decoded_lens
    def broken_triples(d):
        return [t for t in range((len(d) - 4) // 3) if d[3 * t] ^ d[3 * t + 1] != d[3 * t + 2]]

    for label, d in tc.fec_cases("valid"):
        out, ok = tc.ref_fec_decode(d)
        assert ok, label
        if len(d) < 4:
            assert out == d, label
        else:
            nt = (len(d) - 4) // 3
            assert not broken_triples(d), label
            assert out[0:2 * nt:2] == d[0:3 * nt:3] and out[1:2 * nt:2] == d[1:3 * nt:3], label
            assert out[2 * nt:] == d[3 * nt:-4], label
    valid = {len(d): tc.ref_fec_decode(d)[0] for _, d in tc.fec_cases("valid")}
    for v in ("broken_first", "broken_last", "broken_seeded"):
        for label, d in tc.fec_cases(v):
            out, ok = tc.ref_fec_decode(d)
            assert ok, label
            if len(d) < 4:
                continue
            nt = (len(d) - 4) // 3
            broken = broken_triples(d)
            assert len(broken) == 1 and out[2 * broken[0] + 1] == 0x3F, label
            if v != "broken_seeded":
                assert broken[0] == (0 if v == "broken_first" else nt - 1), label
    for v in ("crc_flip", "byte_flip"):
        for label, d in tc.fec_cases(v):
            out, ok = tc.ref_fec_decode(d)
            assert ok == (len(d) < 4), label
            if len(d) >= 4:
                assert not broken_triples(d), label          # the parities still agree: only the CRC objects
    assert all(len(valid[n]) == (n if n < 4 else (n - 4) // 3 * 2 + (n - 4) % 3) for n in tc.FEC_LENGTHS)


def test_frame_families_hold_their_conditions():
    want = {"exact": {"good": tc.OK, "flip": tc.CRC_BAD}, "short": {"good": tc.INCOMPLETE, "flip": tc.INCOMPLETE},
            "long": {"good": tc.OK, "flip": tc.CRC_BAD}}
    fit = tc.frame_fit_cases()
    assert len(fit) == 3 * len(tc.FIT_PAYLOADS) * 6
    for label, raw in fit:
        recs, _, _ = tc.ref_frame_parse(raw)
        _, _, _, tag, cut = label.split("/")
        assert [r["status"] for r in recs] == [want[cut][tag]], label
    for label, raw in tc.frame_header_cases():
        recs, _, _ = tc.ref_frame_parse(raw)
        cut = int(label.rsplit("+", 1)[1])
        st = {29: tc.SHORT, 30: tc.INCOMPLETE, 31: tc.OK, 23: tc.NOMETA, 24: tc.INCOMPLETE, 25: tc.OK}[cut]
        assert [r["status"] for r in recs] == [st], label
    for label, raw in tc.frame_scan_cases():
        recs, frames, _ = tc.ref_frame_parse(raw)
        at = int(label.split("@")[1].split("/")[0])
        if "frame@" in label:
            assert [(r["start"], r["status"]) for r in recs] == [(at, tc.OK)] and len(frames) == 1, label
        else:
            assert len(raw) == at and [(r["start"], r["status"]) for r in recs] == [(at - 4, tc.SHORT)], label
    for mc in tc.CAPS:
        for (label, raw), count in zip(tc.frame_cap_cases(mc), (mc - 1, mc, mc + 1)):
            recs, frames, _ = tc.ref_frame_parse(raw)
            assert len(recs) == count == len(frames) and all(r["status"] == tc.OK for r in recs), label
