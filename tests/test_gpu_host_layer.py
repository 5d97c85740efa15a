"""The host layer of the PSK and FSK plans (csrc/plan_core.h, api.cpp,
fsk_api.cpp), pinned from outside through the C ABI: the four host entries
against the device entry, the edge and soft entries, the timing slots each
pipeline reports, and the error contract -- codes, messages and the order of
the checks.  Every case here passed on the commit before the host layer was
given its shared core; the FSK timing sets are the ones that commit reported."""

import numpy as np
import pytest

from test_gpu_rawint import _raw_batch
from test_gpu_viterbi import Dev

pytestmark = pytest.mark.gpu

B, N, MAXS = 3, 4800, 64
# These filters' time-split design needs n >= 4 warm-ups: at 4800 samples a PSK
# plan forced to "split" runs the row layout.  14800 is the first length on a
# 400-sample grid that amr_psk_split_design accepts for QPSK and BPSK at 9600,
# so the split layout's cases run there; everything else (FSK splits at 4800) at N.
N_SPLIT = 14800
PSK_BAUD = 9600
FSK = (19200, 21000.0, 27000.0)              # sps 5: decision windows of 2 (tests/test_gpu_fsk.py)
PSK_LAYOUTS = ("row", "lane", "split")
FSK_LAYOUTS = ("serial", "split")
POISON = 0xA5


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")


class Case:
    """One plan (max_streams = 64) of a kind ("qpsk", "bpsk", "fsk") at one
    length, its B distinct captures, and the C entry points under common names."""

    def __init__(self, kind, n):
        import _amr
        import _fsk
        import synth
        self.kind, self.fsk, self.n = kind, kind == "fsk", n
        self.L = _amr.lib()
        if self.fsk:
            self.x = synth.fsk_batch(B, n, *FSK, seed=7, distinct=B, noise=0.3)
            self.plan = _fsk.FskPlan(n, *FSK, max_streams=MAXS)
            self.pad = 3 * len(self.plan.coef[0])
        else:
            self.x = synth.qpsk_batch(B, n, PSK_BAUD, seed=5, distinct=B)
            self.plan = _amr.PskPlan(kind, n, PSK_BAUD, max_streams=MAXS)
            self.pad = 3 * len(self.plan.bp[0])
        self.h, self.cap = self.plan.handle, self.plan.out_cap
        self.ref = {}

    def fn(self, name):
        return getattr(self.L, f"amr_{'fsk' if self.fsk else 'psk'}_{name}")

    def ran(self, layout):
        """the layout the last call ran, in set_layout's names"""
        if self.fsk:
            return "split" if self.plan.split_info()["last_split"] else "serial"
        return self.plan.last_layout()

    def device(self, layout, x=None, edges=None):
        """(out [B][cap], len, sync) of _demod_device (or _device_edges) on x uploaded with amr_memcpy_h2d."""
        import _amr
        if edges is None and layout in self.ref:
            return self.ref[layout]
        x = self.x if x is None else x
        self.plan.set_layout(layout)
        with Dev() as d:
            d_x, d_out = d.put(np.ascontiguousarray(x)), d.put(np.full((B, self.cap), POISON, np.uint8))
            d_len, d_sync = d.put(np.zeros(B, np.int64)), d.put(np.zeros(B, np.int64))
            if edges is None:
                _amr.check(self.fn("demod_device")(self.h, d_x, _amr.DTYPES[x.dtype], B, x.shape[1], d_out, self.cap,
                                                   d_len, d_sync))
            else:
                _amr.check(self.fn("demod_device_edges")(self.h, d_x, _amr.DTYPES[x.dtype], B, x.shape[1],
                                                         d.put(edges), d_out, self.cap, d_len, d_sync))
            _amr.check(self.fn("plan_synchronize")(self.h))
            assert self.ran(layout) == layout
            got = (d.get(d_out, np.zeros((B, self.cap), np.uint8)), d.get(d_len, np.zeros(B, np.int64)),
                   d.get(d_sync, np.zeros(B, np.int64)))
        assert got[1].max() > 0 and got[1].max() < self.cap
        if edges is None:
            self.ref[layout] = got
        return got


def rows(out, ln, width=None):
    """each stream's bytes, cut to its row (a row holds up to `width` of them)"""
    return [out[i, :min(ln[i], out.shape[1] if width is None else width)].tobytes() for i in range(len(ln))]


_cases = {}


class Modem:
    """the cases of a kind: at(layout) is the one whose length that layout really runs at"""

    def __init__(self, kind):
        self.kind, self.fsk = kind, kind == "fsk"
        self.layouts = FSK_LAYOUTS if self.fsk else PSK_LAYOUTS

    def at(self, layout):
        key = (self.kind, N_SPLIT if layout == "split" and not self.fsk else N)
        if key not in _cases:
            _cases[key] = Case(*key)
        return _cases[key]


@pytest.fixture
def modem(request):
    return Modem(request.param)


KINDS = pytest.mark.parametrize("modem", ["qpsk", "bpsk", "fsk"], indirect=True)


# ---- 1. the host entries agree with the device entry ----------------------------------
@KINDS
@pytest.mark.parametrize("entry", ["host", "host_async"])
@pytest.mark.parametrize("x_pad", [0, 7])
@pytest.mark.parametrize("out_pad", [0, -1, 5])
def test_host_entries_equal_the_device_entry(modem, entry, x_pad, out_pad):
    import _amr
    for layout in modem.layouts:
        c = modem.at(layout)
        want, wlen, wsync = c.device(layout)
        assert len(set(rows(want, wlen))) == B                              # real, distinct streams
        xs = np.zeros((B, c.n + x_pad), c.x.dtype)
        xs[:, :c.n] = c.x
        stride = c.cap + out_pad
        c.plan.set_layout(layout)
        out = np.full((B, stride), POISON, np.uint8)
        ln, sy = np.full(B, -7, np.int64), np.full(B, -7, np.int64)
        _amr.check(c.fn("demod_" + entry)(c.h, _amr.ptr(xs), _amr.DTYPES[xs.dtype], B, c.n + x_pad, _amr.ptr(out), stride,
                                          _amr.ptr(ln), _amr.ptr(sy)))
        if entry == "host_async":
            _amr.check(c.fn("plan_synchronize")(c.h))
        assert c.ran(layout) == layout
        assert np.array_equal(ln, wlen) and np.array_equal(sy, wsync), layout
        assert rows(out, ln) == rows(want, wlen, stride), layout            # out_len says cap - 1 where the row is cut
        assert np.all(out[:, c.cap:] == POISON), layout                     # nothing past the capacity


# ---- 2. the edge and soft entries -----------------------------------------------------------
@pytest.mark.parametrize("modem", ["qpsk", "fsk"], indirect=True)
def test_host_edges_equals_device_edges(modem):
    import _amr
    rng = np.random.default_rng(17)
    for layout in modem.layouts:
        c = modem.at(layout)
        raw = _raw_batch(rng, "fsk", np.int16, B, c.n, *FSK) if c.fsk else \
            _raw_batch(rng, "qpsk", np.int16, B, c.n, PSK_BAUD, 3000.0, 0.0)
        xk, edges = _amr.raw_input(raw, c.pad)
        want, wlen, wsync = c.device(layout, xk, edges)
        c.plan.set_layout(layout)
        out = np.full((B, c.cap), POISON, np.uint8)
        ln, sy = np.full(B, -7, np.int64), np.full(B, -7, np.int64)
        _amr.check(c.fn("demod_host_edges")(c.h, _amr.ptr(xk), _amr.DTYPES[xk.dtype], B, c.n, _amr.ptr(edges),
                                            _amr.ptr(out), c.cap, _amr.ptr(ln), _amr.ptr(sy)))
        assert c.ran(layout) == layout
        assert np.array_equal(ln, wlen) and np.array_equal(sy, wsync) and rows(out, ln) == rows(want, wlen), layout


def last_calls(plan):
    return plan.last_layout(), plan.last_lowpass(), plan.last_f32f(), plan.last_strict()


@pytest.mark.parametrize("modem", ["qpsk", "bpsk"], indirect=True)
def test_soft_host_equals_soft_device_and_keeps_the_bookkeeping(modem):
    """A soft call runs the row or lane layout and leaves amr_psk_plan_last_*
    as the hard call before it set them (test_gpu_soft.py pins the layout alone)."""
    import _amr
    for layout in PSK_LAYOUTS:
        c = modem.at(layout)
        sstride = 8 * c.cap + 3
        c.plan.set_layout(layout)
        c.plan.set_split_strict(layout == "split")
        hard, _ = c.plan.demod_host(c.x)
        before = last_calls(c.plan)
        assert before[0] == layout and (layout != "lane" or before[1] != "none")
        out, soft = np.full((B, c.cap), POISON, np.uint8), np.full((B, sstride), 0x55, np.int8)
        ln, sy = np.zeros(B, np.int64), np.zeros(B, np.int64)
        _amr.check(c.L.amr_psk_demod_soft_host(c.h, _amr.ptr(c.x), _amr.DTYPE_F32, B, c.n, _amr.ptr(out), c.cap,
                                               _amr.ptr(ln), _amr.ptr(sy), None, _amr.ptr(soft), sstride))
        assert last_calls(c.plan) == before, layout
        with Dev() as d:
            d_x, d_out = d.put(c.x), d.put(np.full((B, c.cap), POISON, np.uint8))
            d_len, d_sync = d.put(np.zeros(B, np.int64)), d.put(np.zeros(B, np.int64))
            d_soft = d.put(np.full((B, sstride), 0x55, np.int8))
            _amr.check(c.L.amr_psk_demod_soft_device(c.h, d_x, _amr.DTYPE_F32, B, c.n, d_out, c.cap, d_len, d_sync,
                                                     None, d_soft, sstride))
            _amr.check(c.L.amr_psk_plan_synchronize(c.h))
            dsoft, dlen = d.get(d_soft, np.zeros((B, sstride), np.int8)), d.get(d_len, np.zeros(B, np.int64))
            dout = d.get(d_out, np.zeros((B, c.cap), np.uint8))
        assert last_calls(c.plan) == before, layout
        c.plan.set_split_strict(None)
        assert np.array_equal(ln, dlen) and rows(out, ln) == rows(dout, dlen) == hard
        for i in range(B):
            assert np.array_equal(soft[i], dsoft[i]) and soft[i, :8 * ln[i]].any(), (layout, i)
            assert np.all(soft[i, 8 * ln[i]:] == 0x55)


# ---- 3. the timing slots, exactly --------------------------------------------------------------
PSK_SLOTS = {"row": {"bandpass", "lowpass_fwd", "lowpass_bwd", "lowpass_exact", "sync_pack", "launch"},
             "lane": {"bandpass", "lowpass_fwd", "lowpass_exact", "sync_pack", "launch"},
             "split": {"bandpass", "lowpass_fwd", "lowpass_exact", "sync_pack", "launch"}}
# what the commit before the shared core reported (serial and split F1 alike;
# "exact" only while the exact path launches: not with exact mode 0)
FSK_SLOTS = {"bandpass", "hilbert", "decide", "launch", "exact"}


@pytest.mark.parametrize("layout", PSK_LAYOUTS)
def test_psk_timing_slots(layout):
    import _amr
    import synth
    n = N_SPLIT if layout == "split" else N
    x = synth.qpsk_batch(B, n, PSK_BAUD, seed=5, distinct=B)
    plan = _amr.PskPlan("qpsk", n, PSK_BAUD, max_streams=MAXS)
    plan.set_layout(layout)
    plan.enable_timing(True)
    plan.demod_host(x)
    assert plan.last_layout() == layout
    assert set(plan.timings()) == PSK_SLOTS[layout]
    cap = plan.out_cap
    with Dev() as d:                                             # + the FEC stage behind the same layout
        d_x, d_out, d_fec = d.put(x), d.put(np.zeros((B, cap), np.uint8)), d.put(np.zeros((B, cap), np.uint8))
        d_len, d_sync, d_flen = (d.put(np.zeros(B, np.int64)) for _ in range(3))
        d_crc = d.put(np.zeros(B, np.int32))
        _amr.check(d.L.amr_psk_demod_fec_device(plan.handle, d_x, _amr.DTYPE_F32, B, n, d_out, cap, d_len, d_sync,
                                                d_fec, cap, d_flen, d_crc))
        assert set(plan.timings()) == PSK_SLOTS[layout] | {"fec"}
    plan.demod_host(x)                                           # and gone again with the next plain call
    assert set(plan.timings()) == PSK_SLOTS[layout]


def test_psk_timing_slots_fewer_than_two_symbols():
    import _amr
    plan = _amr.PskPlan("qpsk", 60, 1000, max_streams=MAXS)
    plan.enable_timing(True)
    outs, sync = plan.demod_host(np.random.default_rng(1).normal(0, 0.3, (B, 60)).astype(np.float32))
    assert outs == [b""] * B and list(sync) == [-1] * B
    assert set(plan.timings()) == {"launch"}


@pytest.mark.parametrize("layout", FSK_LAYOUTS)
def test_fsk_timing_slots(layout):
    import _fsk
    import synth
    x = synth.fsk_batch(B, N, *FSK, seed=7, distinct=B, noise=0.3)
    plan = _fsk.FskPlan(N, *FSK, max_streams=MAXS)
    plan.set_layout(layout)
    plan.enable_timing(True)
    plan.demod_host(x)
    assert plan.split_info()["last_split"] == (layout == "split")
    assert set(plan.timings()) == FSK_SLOTS
    plan.set_exact_mode(0)
    plan.demod_host(x)
    assert set(plan.timings()) == FSK_SLOTS - {"exact"}


# ---- 4. the error contract ------------------------------------------------------------------------
def bad_calls(cap):
    """(what, dtype, B, x_stride, out_stride, x is NULL) -> (code, message)"""
    import _amr
    f32 = _amr.DTYPE_F32
    return [("null x", f32, B, N, cap, True, _amr.AMR_E_INVALID, "NULL argument"),
            ("dtype", 99, B, N, cap, False, _amr.AMR_E_INVALID, "unknown dtype"),
            ("capacity", f32, MAXS + 1, N, cap, False, _amr.AMR_E_CAPACITY, "batch exceeds plan max_streams"),
            ("x_stride", f32, B, N - 1, cap, False, _amr.AMR_E_INVALID, "x_stride < n_samples"),
            ("out_stride", f32, B, N, cap - 2, False, _amr.AMR_E_INVALID, "out_stride too small"),
            ("out_stride 0", f32, B, N, 0, False, _amr.AMR_E_INVALID, "out_stride too small")]


@KINDS
@pytest.mark.parametrize("entry", ["host", "host_async", "device"])
def test_error_contract(modem, entry):
    import _amr
    m = modem.at("row")
    call = m.fn("demod_" + entry)
    name = call.__name__
    out = np.full((B, m.cap), POISON, np.uint8)
    ln, sy = np.full(B, -7, np.int64), np.full(B, -7, np.int64)
    # (no call below gets as far as reading or writing a buffer: host memory serves the device entry too)
    bufs = (_amr.ptr(out), _amr.ptr(ln), _amr.ptr(sy))

    def err(rc, code, msg):
        assert rc == code, (rc, m.L.amr_last_error())
        assert m.L.amr_last_error().decode() == msg

    err(call(None, _amr.ptr(m.x), _amr.DTYPE_F32, B, N, bufs[0], m.cap, *bufs[1:]), _amr.AMR_E_INVALID,
        f"{name}: NULL argument")
    for what, dtype, nb, xst, ost, null_x, code, msg in bad_calls(m.cap):
        rc = call(m.h, None if null_x else _amr.ptr(m.x), dtype, nb, xst, bufs[0], ost, *bufs[1:])
        err(rc, code, f"{name}: {msg}" if null_x else msg)
    # two bad arguments: the host entries test the dtype first, the device entries the capacity
    rc = call(m.h, _amr.ptr(m.x), 99, MAXS + 1, N, bufs[0], m.cap, *bufs[1:])
    if entry == "device":
        err(rc, _amr.AMR_E_CAPACITY, "batch exceeds plan max_streams")
    else:
        err(rc, _amr.AMR_E_INVALID, "unknown dtype")
    # an empty batch: OK, whatever the pointers, and nothing touched
    assert call(m.h, None, _amr.DTYPE_F32, 0, N, None, m.cap, None, None) == _amr.AMR_OK
    assert call(m.h, _amr.ptr(m.x), _amr.DTYPE_F32, 0, N, bufs[0], m.cap, *bufs[1:]) == _amr.AMR_OK
    _amr.check(m.fn("plan_synchronize")(m.h))
    assert np.all(out == POISON) and np.all(ln == -7) and np.all(sy == -7)
