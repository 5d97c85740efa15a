"""The lane band-pass's zero-tap detector watches y (psk_common.h zo_watch_y);
AMR_BP_ZDET=0 keeps the earlier watch of four states.  Which detector runs
decides only which streams take the full-tap fix-up, never a byte: both must
give the oracle's bytes, lengths and sync indices for every stream, and each
other's.

Lane layout forced, float32 input, QPSK at 9600 Bd.  Batches of 65 and 130
streams (whole and ragged groups, an inactive group inside the last
workgroup); lengths 31 (no whole band-pass tile), 33 (one and a one-sample
tail), 69 (two and a tail) and 4000 (125 whole tiles, no tail).  Streams the
detectors have to deal with -- silence, a frame cut off by exact zeros, runs
of -0.0 at the start and inside, float32 denormals of both signs down to
2^-149, an inf, a NaN -- sit at lanes 0, 31, 32 and 63 of otherwise ordinary
groups.  (tests/test_bp_zero_detector.py drives the steps themselves on the
CPU, down to float64 denormals and 2^-1000 scalings no float32 input holds.)

The switches are read once per process: each detector runs in one child
process of its own over the same inputs; the oracle runs once, here."""
import itertools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SETTINGS = {"y": {}, "z": {"AMR_BP_ZDET": "0"}}
BATCHES = (65, 130)
LENGTHS = (31, 33, 69, 4000)
BAUD = 9600
KINDS = ("silence", "cut", "negzero_start", "negzero_inside", "denormals", "inf", "nan")
SWITCHES = ("AMR_BP_ZDET", "AMR_BP_ZO", "AMR_PSK_LANE")


def _spots(B):
    """lanes 0, 31, 32, 63 of every whole group, and the first lane of a ragged last group"""
    s = [g * 64 + lane for g in range(B // 64) for lane in (0, 31, 32, 63)]
    return s + ([B // 64 * 64] if B % 64 else [])


def _spoil(row, kind, rng):
    n = row.size
    if kind == "silence":
        row[:] = 0.0
    elif kind == "cut":
        row[n // 3:] = 0.0
    elif kind == "negzero_start":
        row[:max(2, n // 2)] = -0.0
    elif kind == "negzero_inside":
        row[n // 4:n // 4 + max(2, n // 3)] = -0.0
    elif kind == "denormals":
        m = rng.integers(1, 2 ** 23, n).astype(np.uint32) >> rng.integers(0, 23, n).astype(np.uint32)
        row[:] = np.maximum(m, 1).view(np.float32) * rng.choice(np.float32([-1, 1]), n)
    elif kind == "inf":
        row[n - 5] = np.inf
    elif kind == "nan":
        row[n // 2] = np.nan


def _cases():
    """name -> (x [B][n] float32, the silent streams)"""
    import synth
    c = {}
    for k, (B, n) in enumerate(itertools.product(BATCHES, LENGTHS)):
        x = synth.qpsk_batch(B, n, BAUD, seed=500 + k, distinct=min(B, 7))
        rng = np.random.default_rng(900 + k)
        silent = []
        for j, s in enumerate(_spots(B)):
            kind = KINDS[(j + k) % len(KINDS)] if j else "silence"     # every case has a silent stream at lane 0
            _spoil(x[s], kind, rng)
            if kind == "silence":
                silent.append(s)
        c[f"b{B}_n{n}"] = (x, silent)
    return c


CHILD = '''
import sys, pickle
sys.path[:0] = [{pkg!r}, {root!r}]
import numpy as np
import _amr
inp = np.load({inputs!r})
res = {{}}
for name in {names!r}:
    x = inp[name]
    pl = _amr.PskPlan("qpsk", x.shape[1], {baud!r}, max_streams=x.shape[0])
    got, gs = pl.demod_host(x)
    res[name] = (got, np.asarray(gs), pl.last_layout(), pl.exact_streams())
    del pl
pickle.dump(res, open({out!r}, "wb"))
'''


def _child(tmp, tag, env, names, inputs):
    out = os.path.join(tmp, tag + ".pkl")
    script = os.path.join(tmp, tag + ".py")
    with open(script, "w") as f:
        f.write(CHILD.format(pkg=os.path.join(ROOT, "audio-modem-radio_amd"), root=ROOT, inputs=inputs, names=names,
                             baud=BAUD, out=out))
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env, AMR_PSK_LANE="1")
    r = subprocess.run([sys.executable, script], env=e, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with open(out, "rb") as f:
        return pickle.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(cases, the oracle's outputs, {detector: the child's outputs})"""
    from oracle import oracle
    tmp = str(tmp_path_factory.mktemp("bp_zdet"))
    cases = _cases()
    inputs = os.path.join(tmp, "inputs.npz")
    np.savez(inputs, **{k: v[0] for k, v in cases.items()})
    nt = min(16, os.cpu_count() or 1)
    want = {k: oracle.psk_demod_batch("qpsk", x, BAUD, n_threads=nt) for k, (x, _) in cases.items()}
    got = {s: _child(tmp, s, env, list(cases), inputs) for s, env in SETTINGS.items()}
    return cases, want, got


def test_case_list_is_whole(runs):
    cases = runs[0]
    assert len(cases) == len(BATCHES) * len(LENGTHS)
    assert all(silent and silent[0] == 0 for _, silent in cases.values())


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_bytes_lengths_and_sync_equal_the_oracle(runs, setting):
    cases, want, got = runs
    bad = {}
    for name in cases:
        g, gs, layout, _ = got[setting][name]
        w, ws = want[name]
        assert layout == "lane", name
        assert len(g) == len(w), name
        b = [i for i in range(len(w)) if g[i] != w[i] or len(g[i]) != len(w[i]) or int(gs[i]) != int(ws[i])]
        if b:
            bad[name] = b[:8]
    assert not bad, f"{len(bad)} of {len(cases)} cases differ from the oracle: {bad}"


def test_both_detectors_give_the_same_outputs(runs):
    cases, _, got = runs
    bad = [name for name in cases
           if not (got["y"][name][0] == got["z"][name][0] and np.array_equal(got["y"][name][1], got["z"][name][1]))]
    assert not bad, f"bytes or sync indices differ between the detectors: {bad}"


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_silent_streams_reach_the_exact_path(runs, setting):
    """A silent stream's y is zero from the first step: the band-pass flags it
    (its group is re-run with every tap), its f is all zeros, and the low-pass
    sends it down the exact path, which exact_streams() counts."""
    cases, _, got = runs
    for name, (_, silent) in cases.items():
        assert got[setting][name][3] >= len(silent), name
