"""The receiver's integer tail on the GPU, at every length and offset:
k_sync_pack (through _amr.sync_pack, the stage alone), k_fec_decode and
k_frame_parse against the plain restatements of tests/tail_cases.py -- which
tests/test_tail_cases.py pins, case by case, to the reference's own results.
Each test is a few launches of short streams and names the first (case,
field) that differs."""
import contextlib
import io

import numpy as np
import pytest

import tail_cases as tc

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")


def _differ(label, field, got, want):
    pytest.fail(f"first difference at ({label}, {field}): got {got!r}, want {want!r}")


# ---------------------------------------------------------------------------
# sync search + byte pack
def check_sync(cases, slack=8):
    """One launch per (n_bits, n_words) among the cases, out_stride = n_bits // 8
    + slack: sync index, byte count and bytes are the restatement's, and every
    byte of `out` at or past out_len is still the fill value."""
    import _amr
    groups = {}
    for i, (_, row, n, nw) in enumerate(cases):
        groups.setdefault((n, nw, row.size), []).append(i)
    for (n, nw, _), members in groups.items():
        bits = np.stack([cases[i][1] for i in members])
        out, ln, sy = _amr.sync_pack(bits, n_words=nw, out_stride=n // 8 + slack, fill=FILL, n_bits=n)
        assert out.shape == (len(members), n // 8 + slack)
        for j, i in enumerate(members):
            label = cases[i][0]
            want, idx = tc.ref_sync_pack(cases[i][1][:n])
            if int(sy[j]) != idx:
                _differ(label, "sync_idx", int(sy[j]), idx)
            if int(ln[j]) != len(want):
                _differ(label, "out_len", int(ln[j]), len(want))
            if out[j, :len(want)].tobytes() != want:
                k = next(k for k in range(len(want)) if out[j, k] != want[k])
                _differ(label, f"byte {k}", int(out[j, k]), want[k])
            if not (out[j, len(want):] == FILL).all():
                k = len(want) + int(np.argmax(out[j, len(want):] != FILL))
                _differ(label, f"byte {k} (past out_len {len(want)})", int(out[j, k]), FILL)


def test_sync_at_every_length_and_offset():
    """n_bits 0..160 x a sync at every p in 0..n_bits-16, zero and random filler."""
    check_sync(tc.sync_sweep_cases())


def test_sync_cut_by_one_bit_is_not_completed_from_stale_bits():
    """The pattern starts at n_bits - 15; the missing bit, the rest of the last
    word and (second half) three more words would complete it if read."""
    cases = tc.sync_cut_cases()
    assert all(tc.ref_sync_pack(row[:n])[1] == -1 for _, row, n, _ in cases)
    check_sync(cases)


def test_sync_across_the_search_passes():
    """Rows of 2048 .. 6200 bits: a sync at every p within 40 bits of the 64-word
    pass boundaries, at the last legal p, and none."""
    check_sync(tc.sync_long_cases())


def test_first_of_two_syncs_wins():
    check_sync(tc.sync_two_cases())


def test_pack_widths_and_nothing_past_out_len():
    """Byte counts 0..9, 253..260, 509..516 from a sync at bit 0 / 5 / 31 / 37 or
    from bit 0 without one; out_stride leaves 8 and more bytes that must stay."""
    check_sync(tc.sync_pack_cases())


def test_sync_random_rows():
    check_sync(tc.sync_random_cases())


# ---------------------------------------------------------------------------
# the same stage behind the real demodulators
def _consecutive(sync):
    s = sorted(int(v) for v in sync)
    return s == list(range(s[0], s[0] + len(s)))


@pytest.mark.parametrize("layout", ["row", "lane", "split"])
def test_qpsk_companion_streams(layout):
    """64 QPSK @ 1000 Bd streams whose sync sits k = 0..63 bits into the payload:
    bytes and sync index are the oracle's, and the indices are 64 consecutive values."""
    import _amr
    import modem
    from oracle import oracle
    x = modem.modulate_batch("qpsk", tc.companion_payloads(), tc.COMPANION_PSK_BAUD)
    want, wsync = oracle.psk_demod_batch("qpsk", x, tc.COMPANION_PSK_BAUD)
    assert _consecutive(wsync), list(wsync)
    plan = _amr.PskPlan("qpsk", x.shape[1], tc.COMPANION_PSK_BAUD, max_streams=x.shape[0])
    if layout == "lane":
        plan.set_inflight(1024)
    else:
        plan.set_layout(layout)
    got, gsync = plan.demod_host(x)
    assert plan.last_layout() == layout or (layout == "split" and plan.last_layout() == "row")
    for k in range(len(want)):
        if int(gsync[k]) != int(wsync[k]):
            _differ(f"companion/qpsk/{layout}/k{k}", "sync_idx", int(gsync[k]), int(wsync[k]))
        if got[k] != want[k]:
            _differ(f"companion/qpsk/{layout}/k{k}", "bytes", got[k].hex(), want[k].hex())
    assert _consecutive(gsync)


@pytest.mark.parametrize("layout", ["auto", "serial", "split"])
def test_fsk_companion_streams(layout):
    """The same 64 payloads through FSK @ 1200 Bd, 2400 / 4800 Hz, in each F1 layout."""
    import _fsk
    import modem
    from oracle import oracle
    baud, mark, space = tc.COMPANION_FSK
    x = modem.modulate_batch("fsk", tc.companion_payloads(), baud, mark, space)
    res = [oracle.fsk_demodulate(r, baud, mark, space, return_sync=True) for r in x]
    want, wsync = [r[0] for r in res], [r[1] for r in res]
    assert _consecutive(wsync), wsync
    plan = _fsk.FskPlan(x.shape[1], baud, mark, space, max_streams=x.shape[0])
    plan.set_layout(layout)
    got, gsync = plan.demod_host(x)
    for k in range(len(want)):
        if int(gsync[k]) != wsync[k]:
            _differ(f"companion/fsk/{layout}/k{k}", "sync_idx", int(gsync[k]), wsync[k])
        if got[k] != want[k]:
            _differ(f"companion/fsk/{layout}/k{k}", "bytes", got[k].hex(), want[k].hex())
    assert _consecutive(gsync)


# ---------------------------------------------------------------------------
# FEC decode
@pytest.mark.parametrize("variant", tc.FEC_VARIANTS)
def test_fec_every_length(variant):
    """Every input length 0..800 in one ragged batch, 4099 / 65 541 / 200 003 in
    a second one (their rows are wide): decoded bytes and CRC verdict."""
    import fec
    cases = tc.fec_cases(variant)
    for group in ([c for c in cases if len(c[1]) <= 800], [c for c in cases if len(c[1]) > 800]):
        outs, oks = fec.ReedSolomonFEC().decode_batch([d for _, d in group])
        assert len(outs) == len(oks) == len(group)
        for (label, d), out, ok in zip(group, outs, oks):
            want, wok = tc.ref_fec_decode(d)
            if len(out) != len(want):
                _differ(label, "out_len", len(out), len(want))
            if out != want:
                k = next(k for k in range(len(want)) if out[k] != want[k])
                _differ(label, f"byte {k}", out[k], want[k])
            if bool(ok) != wok:
                _differ(label, "crc_ok", bool(ok), wok)


# ---------------------------------------------------------------------------
# frame parse
def _batches(cases, limit=1024):
    """Short streams in one launch, long ones in another (rows are padded to the longest)."""
    return [g for g in ([c for c in cases if len(c[1]) <= limit], [c for c in cases if len(c[1]) > limit]) if g]


def check_records(cases, max_cands):
    import _amr
    for group in _batches(cases):
        res = _amr.frame_parse([raw for _, raw in group], max_cands=max_cands)
        for (label, raw), (count, recs) in zip(group, res):
            want, _, _ = tc.ref_frame_parse(raw)
            if count != len(want):
                _differ(label, "n_cands", count, len(want))
            if len(recs) != min(len(want), max_cands):
                _differ(label, "records kept", len(recs), min(len(want), max_cands))
            for k, (r, w) in enumerate(zip(recs, want)):
                fields = tc.REC_FIELDS + (("calc_crc",) if w["status"] in (tc.OK, tc.CRC_BAD) else ())
                for f in fields:
                    if int(r[f]) != w[f]:
                        _differ(label, f"record {k} {f}", int(r[f]), w[f])


def check_dropin(cases, max_cands):
    import decoder
    for group in _batches(cases):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            got = decoder.parse_fbp_stream_enhanced_batch([raw for _, raw in group], max_cands=max_cands)
        logs = ["Encontrados " + part for part in buf.getvalue().split("Encontrados ")[1:]]
        assert len(got) == len(logs) == len(group)
        for (label, raw), frames, log in zip(group, got, logs):
            _, wframes, wlog = tc.ref_frame_parse(raw)
            if len(frames) != len(wframes):
                _differ(label, "frames", len(frames), len(wframes))
            for k, (f, w) in enumerate(zip(frames, wframes)):
                for key in ("name", "data", "final_crc"):
                    if f[key] != w[key]:
                        _differ(label, f"frame {k} {key}", f[key], w[key])
            if log != wlog:
                _differ(label, "log", log, wlog)


@pytest.mark.parametrize("family", ["frame_fit", "frame_header", "frame_scan"])
def test_frame_records(family):
    """Exact-fit, one byte short and one byte long streams (payloads 1..200 and
    around 256, 4096, 65 536; names of 1, 2, 255 bytes), streams cut at the two
    header checks, frames and bare magics across the 64-byte scan blocks."""
    check_records(tc.frame_families()[family], max_cands=8)


@pytest.mark.parametrize("family", ["frame_fit", "frame_header", "frame_scan"])
def test_frame_dropin(family):
    check_dropin(tc.frame_families()[family], max_cands=8)


@pytest.mark.parametrize("max_cands", tc.CAPS)
def test_frame_candidate_caps(max_cands):
    """max_cands - 1, max_cands and max_cands + 1 short valid frames: the count is
    the true one, the records are the first min(count, max_cands) in order, and
    the drop-in gives the restatement's frames and log in all three."""
    cases = tc.frame_cap_cases(max_cands)
    check_records(cases, max_cands)
    check_dropin(cases, max_cands)
