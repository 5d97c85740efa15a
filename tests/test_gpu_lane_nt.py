"""The lane kernels' cache policies (AMR_LANE_NT: which of their streamed
accesses go non-temporal) and the scope of the fence after their forward
passes (AMR_LANE_FENCE) change how bytes move, never which bytes: every
setting must give the oracle's bytes, lengths and sync indices, and the very
outputs of mask 0.

The AMR_* switches are read once per process, so every setting runs in one
child process of its own over the same inputs (written once to a file); the
oracle runs once, here.  Settings: mask 0 (the default policy everywhere),
the built-in default (no AMR_LANE_NT in the environment), 31 (every class
non-temporal) and the default with the device-scope fence, each with the
fused slicer forced on (k_lp_lane_h) and off (k_lp_lane + K4a)."""
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

SETTINGS = {"nt0": {"AMR_LANE_NT": "0"}, "default": {}, "nt31": {"AMR_LANE_NT": "31"},
            "default_devfence": {"AMR_LANE_FENCE": "1"}}
FUSE = ("1", "0")
# batches: a lone lane, a full group, a one-lane second group, a partial second half of k_lp_lane_h's (group, half)
BATCHES = (1, 64, 65, 130)
# one low-pass tile only; whole band-pass tiles + a low-pass tail; whole low-pass tiles, no tail; both tails
LENGTHS = (79, 96, 1000, 4007)
MODES = {"qpsk9600": ("qpsk", 9600), "qpsk19200": ("qpsk", 19200), "bpsk4800": ("bpsk", 4800)}   # sps 10, 5, 20
DTYPES = ("f32", "f64", "i16")
# the flagged case: stream -> what the detectors must catch, below and above lane 32 of ordinary groups
FLAG_AT = {3: "silence", 40: "negzero", 65: "inf", 129: "nan"}


def _as(x, dt):
    if dt == "f64":
        return x.astype(np.float64)
    if dt == "i16":
        return (x * 20000).astype(np.int16)
    return x


def _cases():
    """name -> (kind, baud, x)"""
    import synth
    c = {}
    for (mode, (kind, baud)), B, n in itertools.product(MODES.items(), BATCHES, LENGTHS):
        x = synth.qpsk_batch(B, n, baud, seed=1000 + 7 * B + n, distinct=min(B, 5))
        for dt in DTYPES:
            c[f"{mode}_b{B}_n{n}_{dt}"] = (kind, baud, _as(x, dt))
    x = synth.qpsk_batch(130, 4007, 9600, seed=12, distinct=9)
    x[3] = 0.0
    x[40, :3000] = -0.0
    x[65, 4000] = np.inf
    x[129, 1234] = np.nan
    c["flagged"] = ("qpsk", 9600, x)
    return c


CHILD = '''
import sys, pickle
sys.path[:0] = [{pkg!r}, {root!r}]
import numpy as np
import _amr
inp = np.load({inputs!r})
res = {{}}
for name, kind, baud in {cases!r}:
    x = inp[name]
    pl = _amr.PskPlan(kind, x.shape[1], baud, max_streams=x.shape[0])
    got, gs = pl.demod_host(x)
    res[name] = (got, np.asarray(gs), pl.last_layout(), pl.last_lowpass(), pl.exact_streams())
    del pl
pickle.dump(res, open({out!r}, "wb"))
'''

SWITCHES = ("AMR_LANE_NT", "AMR_LANE_FENCE", "AMR_LP_HALF", "AMR_FUSED_SLICE", "AMR_PSK_LANE")


def _child(tmp, tag, env, cases, inputs):
    out = os.path.join(tmp, tag + ".pkl")
    script = os.path.join(tmp, tag + ".py")
    with open(script, "w") as f:
        f.write(CHILD.format(pkg=os.path.join(ROOT, "audio-modem-radio_amd"), root=ROOT, inputs=inputs, cases=cases, out=out))
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    r = subprocess.run([sys.executable, script], env=e, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with open(out, "rb") as f:
        return pickle.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(cases, the oracle's outputs, {(setting, fuse): the child's outputs})"""
    from oracle import oracle
    tmp = str(tmp_path_factory.mktemp("lane_nt"))
    cases = _cases()
    inputs = os.path.join(tmp, "inputs.npz")
    np.savez(inputs, **{k: v[2] for k, v in cases.items()})
    names = [(k, v[0], v[1]) for k, v in cases.items()]
    nt = min(16, os.cpu_count() or 1)
    want = {k: oracle.psk_demod_batch(kind, x, baud, n_threads=nt) for k, (kind, baud, x) in cases.items()}
    got = {(s, fu): _child(tmp, f"{s}_fuse{fu}", dict(env, AMR_PSK_LANE="1", AMR_FUSED_SLICE=fu), names, inputs)
           for s, env in SETTINGS.items() for fu in FUSE}
    return cases, want, got


def test_case_list_is_whole(runs):
    assert len(runs[0]) == len(MODES) * len(BATCHES) * len(LENGTHS) * len(DTYPES) + 1


@pytest.mark.parametrize("fuse", FUSE)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_bytes_and_sync_equal_the_oracle(runs, setting, fuse):
    cases, want, got = runs
    bad = {}
    for name in cases:
        g, gs, layout, lp, _ = got[(setting, fuse)][name]
        w, ws = want[name]
        assert (layout, lp) == ("lane", "lane_half" if fuse == "1" else "lane"), name
        b = [i for i in range(len(w)) if g[i] != w[i] or int(gs[i]) != int(ws[i])]
        if b:
            bad[name] = b[:8]
    assert not bad, f"{len(bad)} of {len(cases)} cases differ from the oracle: {dict(list(bad.items())[:6])}"


@pytest.mark.parametrize("fuse", FUSE)
@pytest.mark.parametrize("setting", [s for s in SETTINGS if s != "nt0"])
def test_every_setting_equals_mask_0(runs, setting, fuse):
    cases, _, got = runs
    bad = []
    for name in cases:
        a, b = got[(setting, fuse)][name], got[("nt0", fuse)][name]
        if not (a[0] == b[0] and np.array_equal(a[1], b[1]) and a[4] == b[4]):
            bad.append(name)
    assert not bad, f"{len(bad)} cases differ from mask 0 (bytes, sync indices or exact-path streams): {bad[:8]}"


@pytest.mark.parametrize("fuse", FUSE)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_flagged_streams_reach_the_exact_path(runs, setting, fuse):
    """A silent row, a run of -0.0, a late inf and a NaN inside ordinary
    groups, so that the full-tap fix-up, K3x and K4a read what the
    non-temporal stores wrote (their bytes are compared with the oracle's
    above).  The silent row (f is all zeros), the inf and the NaN (spread over
    the whole stream by the backward passes) must reach the low-pass's exact
    path, which exact_streams() counts; the -0.0 run is the band-pass
    fix-up's alone (3000 samples are far too few for f to decay below the
    low-pass detector's 2^-1015).  The count is the same under every setting."""
    _, _, got = runs
    n = got[(setting, fuse)]["flagged"][4]
    assert n >= sum(1 for what in FLAG_AT.values() if what != "negzero")
    assert n == got[("nt0", fuse)]["flagged"][4]
