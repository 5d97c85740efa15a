"""The half-wave fused low-pass (k_lp_lane_h: re and im of 32 streams in one
wave, the slicer inline, no barrier) against the oracle and against the
two-wave fused kernel it replaces (k_lp_lane FUSE), AMR_LP_HALF=1 / 0.

The AMR_* switches are read once per process, so every variant runs in one
child process of its own over the same inputs (written once to a file); the
oracle runs once, here, and both variants are compared with it byte for byte
(sync indices included) and with each other."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# the streams of FLAGGED the low-pass detector must hand to the exact path:
# index -> what is wrong with it.  Indices below and above 32 of a group
# (3 / 40, 64 / 65 and, in the ragged last group, 129 = its lane 1).
FLAG_AT = {3: "silence", 40: "negzero", 64: "zero", 65: "inf", 129: "nan"}


def _cases():
    """name -> (kind, baud, x).  QPSK@9600 is sps 10: B around the 32 / 64
    stream boundaries of a wave and a group (a wave with one live stream, an
    idle second wave, an idle second group of a workgroup, a ragged last
    group), n below one 40-sample tile and 2 / 3 tiles plus a tail."""
    import synth
    c = {}
    for B in (1, 31, 32, 33, 64, 65, 97, 130):
        c[f"qpsk9600_b{B}"] = ("qpsk", 9600, synth.qpsk_batch(B, 20011, 9600, seed=100 + B, distinct=min(B, 7)))
    for n in (39, 81, 121):
        c[f"qpsk9600_n{n}"] = ("qpsk", 9600, synth.qpsk_batch(65, n, 9600, seed=200 + n, distinct=5))
    c["sps5"] = ("qpsk", 19200, synth.dpsk8_batch(65, 24000, 19200, seed=7, distinct=5))
    c["sps20"] = ("qpsk", 4800, synth.qpsk_batch(33, 30001, 4800, seed=8, distinct=5))
    c["bpsk9600"] = ("bpsk", 9600, synth.qpsk_batch(70, 20000, 9600, seed=6, distinct=3))
    c["bpsk1200"] = ("bpsk", 1200, synth.qpsk_batch(9, 30000, 1200, seed=5, distinct=3))
    x = synth.qpsk_batch(97, 20011, 9600, seed=4, distinct=7)
    c["f64"] = ("qpsk", 9600, x.astype(np.float64))
    c["int16"] = ("qpsk", 9600, (x * 20000).astype(np.int16))
    # 96000 samples: the band-pass's slowest poles (radius 0.98867 at 9600 Bd) take 61 761 samples to
    # carry an amplitude of 1 below the detector's 2^-1015, so 80 000 silent samples leave it 18 000
    x = synth.qpsk_batch(130, 96000, 9600, seed=11, distinct=9)
    x[3, :80000] = 0.0
    x[40, :80000] = -0.0
    x[64] = 0.0
    x[65, 95999] = np.inf
    x[129, 12345] = np.nan
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
    if {inflight!r}:
        pl.set_inflight({inflight!r})
    got, gs = pl.demod_host(x)
    res[name] = (got, np.asarray(gs), pl.last_layout(), pl.last_lowpass(), pl.exact_streams())
pickle.dump(res, open({out!r}, "wb"))
'''


def _child(tmp, tag, env, cases, inputs, inflight=0):
    out = os.path.join(tmp, tag + ".pkl")
    script = os.path.join(tmp, tag + ".py")
    with open(script, "w") as f:
        f.write(CHILD.format(pkg=os.path.join(ROOT, "audio-modem-radio_amd"), root=ROOT, inputs=inputs, cases=cases,
                             inflight=inflight, out=out))
    e = {k: v for k, v in os.environ.items() if k not in ("AMR_LP_HALF", "AMR_FUSED_SLICE", "AMR_PSK_LANE")}
    e.update(env)
    r = subprocess.run([sys.executable, script], env=e, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with open(out, "rb") as f:
        return pickle.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(cases, the oracle's outputs, {variant: the child's outputs})"""
    from oracle import oracle
    tmp = str(tmp_path_factory.mktemp("lp_half"))
    cases = _cases()
    inputs = os.path.join(tmp, "inputs.npz")
    np.savez(inputs, **{k: v[2] for k, v in cases.items()})
    names = [(k, v[0], v[1]) for k, v in cases.items()]
    nt = min(16, os.cpu_count() or 1)
    want = {k: oracle.psk_demod_batch(kind, x, baud, n_threads=nt) for k, (kind, baud, x) in cases.items()}
    forced = {"AMR_PSK_LANE": "1", "AMR_FUSED_SLICE": "1"}
    got = {"half": _child(tmp, "half", dict(forced, AMR_LP_HALF="1"), names, inputs),
           "two_wave": _child(tmp, "two_wave", dict(forced, AMR_LP_HALF="0"), names, inputs),
           # no switch at all: enough streams in flight for the lane layout and its fused slicer
           "auto": _child(tmp, "auto", {}, [n for n in names if n[0] == "qpsk9600_b130"], inputs, inflight=1000)}
    return cases, want, got


CASE_NAMES = ["qpsk9600_b1", "qpsk9600_b31", "qpsk9600_b32", "qpsk9600_b33", "qpsk9600_b64", "qpsk9600_b65",
              "qpsk9600_b97", "qpsk9600_b130", "qpsk9600_n39", "qpsk9600_n81", "qpsk9600_n121", "sps5", "sps20",
              "bpsk9600", "bpsk1200", "f64", "int16", "flagged"]


def test_case_list_is_whole(runs):
    assert sorted(runs[0]) == sorted(CASE_NAMES)


@pytest.mark.parametrize("variant,kernel", [("half", "lane_half"), ("two_wave", "lane_fused")])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_bytes_and_sync_equal_the_oracle(runs, name, variant, kernel):
    _, want, got = runs
    g, gs, layout, lp, _ = got[variant][name]
    w, ws = want[name]
    # 1200 Bd is sps 80: no static symbol slots, so neither fused kernel (the generic k_lp_lane, whatever the switch)
    assert (layout, lp) == ("lane", "lane" if name == "bpsk1200" else kernel)
    bad = [i for i in range(len(w)) if g[i] != w[i] or int(gs[i]) != int(ws[i])]
    assert not bad, f"{len(bad)} of {len(w)} streams differ from the oracle, first {bad[:8]}"


@pytest.mark.parametrize("name", CASE_NAMES)
def test_variants_equal_each_other(runs, name):
    _, _, got = runs
    a, b = got["half"][name], got["two_wave"][name]
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert a[4] == b[4], f"streams sent to the exact path: {a[4]} (half) vs {b[4]} (two-wave)"


def test_flagged_streams_reach_the_exact_path(runs):
    """Streams the detector cannot vouch for, at lanes below and above 32 of
    ordinary groups: an all-zero stream, 80 000 samples of leading +0.0 / -0.0
    silence (the band-pass's forward pass is exactly zero there and its
    backward pass decays into it, below the detector's 2^-1015 after 61 761
    samples and on through denormals to zeros), a late inf and a NaN (both
    spread over the whole stream by the backward passes).  Each raises its own
    stream's flag, so exact_streams() counts at least these five, and the
    same number whichever kernel ran."""
    _, _, got = runs
    n_half, n_two = got["half"]["flagged"][4], got["two_wave"]["flagged"][4]
    print("exact-path streams:", n_half, n_two)
    assert n_half >= len(FLAG_AT)
    assert n_half == n_two


def test_default_selection_is_the_half_wave_kernel(runs):
    """No AMR_LP_HALF, AMR_FUSED_SLICE or AMR_PSK_LANE in the environment:
    with enough batches in flight for the fused slicer, the low-pass that
    runs is k_lp_lane_h, and its bytes are the oracle's."""
    _, want, got = runs
    g, gs, layout, lp, _ = got["auto"]["qpsk9600_b130"]
    assert (layout, lp) == ("lane", "lane_half")
    w, ws = want["qpsk9600_b130"]
    assert g == w and np.array_equal(gs, ws)
