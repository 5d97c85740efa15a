"""modem.py -- drop-in for the reference's modem module, demodulators on MI355X.

Same names and signatures as szumanski/Audio-Modem-Radio modem.py, so
decoder.py / encoder.py / filebeep_advanced_v2.py import it unchanged
(put this directory first on sys.path).  Every demodulator runs on the GPU
through libamr.so (see _amr.py); there is no CPU fallback.

Receive side (the hot path, bit-exact with the reference):
  qpsk_demodulate   modem.py:189-266     bpsk_demodulate  modem.py:68-135
  psk8_demodulate   modem.py:348         ofdm_demodulate_simple modem.py:375-376
  psk31_demodulate  modem.py:397         fsk_demodulate   modem.py:298-341
  fsk_high_speed_demodulate modem.py:355-356   ft8_demodulate modem.py:391
plus batched forms (*_demodulate_batch) that take a [B, N] array and return
one bytes object per stream -- the form the GPU is built for.

d8psk (no reference counterpart): a real 8-ary differential
PSK modem, 3 bits per symbol, beside the psk8_* aliases the reference keeps:
  d8psk_modulate, d8psk_demodulate (+ _batch, _soft, _soft_batch).

star16 (no reference counterpart): a real two-ring 16-DAPSK
modem, 4 bits per symbol (a ring toggle and d8psk's tribit), beside the
apsk16_modulate alias the reference keeps (a QPSK call):
  star16_modulate, star16_demodulate (+ _batch, _soft, _soft_batch).

ofdm (no reference counterpart): a real multi-carrier DQPSK
modem beside the ofdm_*_simple aliases the reference keeps:
  ofdm_modulate, ofdm_demodulate (+ _batch, _soft, _soft_batch).
  A capture that does not start on a symbol boundary:
  ofdm_acquire (+ _batch) finds the boundary from the cyclic prefix, and the
  demodulators' acquire=True reads every stream from its own (a symbol of
  fewer than 8 samples has no prefix: nothing is acquired, the offset is 0).

spread (no reference counterpart): a real direct-sequence
DBPSK modem beside the dsss_modulate alias the reference keeps (a BPSK call):
  spread_modulate, spread_demodulate (+ _batch, _soft, _soft_batch), which
  acquire the code phase of a capture that starts anywhere by default, and
  spread_acquire (+ _batch), the acquisition alone.

minshift (no reference counterpart): a real MSK modem beside
the msk_modulate alias the reference keeps (an FSK call, modulation index 1):
  minshift_modulate, minshift_demodulate (+ _batch, _soft, _soft_batch), which
  recover the bit timing of a capture that starts anywhere by default, and
  minshift_acquire (+ _batch), the bit timing alone.

tone8 (no reference counterpart): a real 8-FSK modem with
Costas sync beside the ft8_* aliases the reference keeps (two-tone FSK calls):
  tone8_modulate, tone8_demodulate (+ _batch, _soft, _soft_batch), which find
  where a capture's frame starts and how far its tones are off the receiver's
  carrier by default, and tone8_acquire (+ _batch), that search alone.

Transmit side (on the GPU: tx_kernels.hip):
  qpsk_modulate modem.py:138-186   bpsk_modulate modem.py:28-65
  fsk_modulate  modem.py:270-295   (+ aliases) and modulate_batch; the float32
  samples equal the reference's up to the last-ulp sin difference the tests bound.
  wav_from_array modem.py:360-368 (host WAV writer).

Hellschreiber (hellschreiber.py, modem.py:400-403), both directions on the GPU:
  feld_hell_demodulate (+ feld_hell_demodulate_batch)  hell_kernels.hip: the
  per-pixel np.mean(chunk ** 2) > 0.1 in numpy's summation order and dtypes,
  bit for bit, then the 7-pixel glyph lookup;
  feld_hell_modulate / hellschreiber_modulate / modulate_batch("hell", ...).
"""
from __future__ import annotations

import numpy as np

import _amr
import synth

SAMPLE_RATE = 96000


class AdvancedModem:
    """modem.py:14-22 (holds the sample rate; AGC helper)."""

    def __init__(self):
        self.sample_rate = SAMPLE_RATE

    def _adaptive_gain_control(self, data: np.ndarray) -> np.ndarray:
        max_val = np.max(np.abs(data))
        if max_val > 0:
            return data / max_val * 0.95
        return data


# ---------------------------------------------------------------------------
# input normalisation
def _as_batch(samples) -> np.ndarray:
    """The caller's samples as an array, in THEIR dtype: the reference hands
    them to filtfilt as they are (modem.py:77, 198, 308), which forms its odd
    extension 2*x[0] - x[k] in that dtype -- a full-scale int16 capture's
    extension wraps.  float32 / float64 go to the kernels as they are; other
    real dtypes (integers of every width, bool, float16) go with the extension
    numpy forms in their own dtype (_amr.raw_input);
    anything else as float64."""
    x = np.asarray(samples)
    if not _amr.is_kernel_dtype(x.dtype) and x.dtype.kind not in "biuf":
        x = x.astype(np.float64)
    return x


def _psk_batch(kind: str, x2d: np.ndarray, baud, carrier, samp_rate):
    if x2d.ndim != 2:
        raise ValueError("batch input must be a 2-D [streams, samples] array")
    x2d = _as_batch(x2d)
    B, n = x2d.shape
    if B == 0:
        return []
    plan = _amr.get_psk_plan(kind, n, baud, carrier, samp_rate, B)
    outs, _ = plan.demod_host(x2d) if _amr.is_kernel_dtype(x2d.dtype) else plan.demod_host_raw(x2d)
    return outs


# 16-bit WAV samples straight from the file (decoder.decode_wav_file): the
# plans take int16 as pcm / 32768 -- exactly the float64 libsndfile gives the
# reference -- so a quarter of the float64 bytes cross PCIe.  Internal: the
# public functions treat integer input as raw values, as the reference does
# (its odd extension wrapping in the integer dtype included).
def _pcm16_psk(kind: str, pcm: np.ndarray, baud, carrier=3000.0, samp_rate=96000) -> bytes:
    x = np.ascontiguousarray(pcm, np.int16)[None, :]
    plan = _amr.get_psk_plan(kind, x.shape[1], baud, carrier, samp_rate, 1)
    return plan.demod_host(x)[0][0]


def _pcm16_fsk(pcm: np.ndarray, baud, mark_freq=1200.0, space_freq=2200.0, samp_rate=96000) -> bytes:
    import _fsk
    return _fsk.fsk_demodulate_batch(np.ascontiguousarray(pcm, np.int16)[None, :], baud, mark_freq, space_freq,
                                     samp_rate)[0]


# ---------------------------------------------------------------------------
# PSK receive side
def qpsk_demodulate(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000) -> bytes:
    """DQPSK demodulation of one stream (modem.py:189-266), on the GPU."""
    x = _as_batch(samples)
    if x.ndim != 1:
        raise ValueError("qpsk_demodulate expects a 1-D sample array (use qpsk_demodulate_batch)")
    return _psk_batch("qpsk", x[None, :], baud, carrier, samp_rate)[0]


def bpsk_demodulate(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000) -> bytes:
    """DBPSK demodulation of one stream (modem.py:68-135), on the GPU."""
    x = _as_batch(samples)
    if x.ndim != 1:
        raise ValueError("bpsk_demodulate expects a 1-D sample array (use bpsk_demodulate_batch)")
    return _psk_batch("bpsk", x[None, :], baud, carrier, samp_rate)[0]


def qpsk_demodulate_batch(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000) -> list:
    """[B, N] equal-length streams -> B bytes objects (each == qpsk_demodulate(row))."""
    return _psk_batch("qpsk", np.asarray(samples), baud, carrier, samp_rate)


def bpsk_demodulate_batch(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000) -> list:
    return _psk_batch("bpsk", np.asarray(samples), baud, carrier, samp_rate)


# soft-decision output (no reference counterpart): the same
# bytes, and one int8 per bit of them -- > 0 bit 1, < 0 bit 0, |v| in 1..127
# how far the differential product lies from the bit's decision boundary --
# for fec.ViterbiDecoder.decode_soft_batch
def _psk_soft_batch(kind: str, x2d: np.ndarray, baud, carrier, samp_rate):
    if x2d.ndim != 2:
        raise ValueError("batch input must be a 2-D [streams, samples] array")
    x2d = _as_batch(x2d)
    B, n = x2d.shape
    if B == 0:
        return [], []
    plan = _amr.get_psk_plan(kind, n, baud, carrier, samp_rate, B)
    outs, _, softs = (plan.demod_soft_host(x2d) if _amr.is_kernel_dtype(x2d.dtype)
                      else plan.demod_soft_host_raw(x2d))
    return outs, softs


def qpsk_demodulate_soft(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000):
    """qpsk_demodulate's bytes and their soft values: (bytes, int8 array of 8 * len(bytes))."""
    x = _as_batch(samples)
    if x.ndim != 1:
        raise ValueError("qpsk_demodulate_soft expects a 1-D sample array (use qpsk_demodulate_soft_batch)")
    outs, softs = _psk_soft_batch("qpsk", x[None, :], baud, carrier, samp_rate)
    return outs[0], softs[0]


def bpsk_demodulate_soft(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000):
    """bpsk_demodulate's bytes and their soft values: (bytes, int8 array of 8 * len(bytes))."""
    x = _as_batch(samples)
    if x.ndim != 1:
        raise ValueError("bpsk_demodulate_soft expects a 1-D sample array (use bpsk_demodulate_soft_batch)")
    outs, softs = _psk_soft_batch("bpsk", x[None, :], baud, carrier, samp_rate)
    return outs[0], softs[0]


def qpsk_demodulate_soft_batch(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000):
    """[B, N] equal-length streams -> (B bytes objects, B int8 arrays)."""
    return _psk_soft_batch("qpsk", np.asarray(samples), baud, carrier, samp_rate)


def bpsk_demodulate_soft_batch(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000):
    return _psk_soft_batch("bpsk", np.asarray(samples), baud, carrier, samp_rate)


# ---------------------------------------------------------------------------
# d8psk: 8-ary differential PSK.  QPSK's front end (band-pass
# carrier +- 1.5 baud, low-pass baud / nyquist, first sample at sps // 2), an
# eight-sector slicer with Gray-coded tribits, the same sync search.
def d8psk_demodulate(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000) -> bytes:
    """8-ary differential PSK demodulation of one stream, on the GPU."""
    x = _as_batch(samples)
    if x.ndim != 1:
        raise ValueError("d8psk_demodulate expects a 1-D sample array (use d8psk_demodulate_batch)")
    return _psk_batch("d8psk", x[None, :], baud, carrier, samp_rate)[0]


def d8psk_demodulate_batch(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000) -> list:
    """[B, N] equal-length streams -> B bytes objects (each == d8psk_demodulate(row))."""
    return _psk_batch("d8psk", np.asarray(samples), baud, carrier, samp_rate)


def d8psk_demodulate_soft(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000):
    """d8psk_demodulate's bytes and their soft values: (bytes, int8 array of 8 * len(bytes)).
    Three values per symbol, b2, b1, b0; b0's magnitude tops out near 74, not 127
    (its decision lines lie pi/4 apart, the other bits' pi/2)."""
    x = _as_batch(samples)
    if x.ndim != 1:
        raise ValueError("d8psk_demodulate_soft expects a 1-D sample array (use d8psk_demodulate_soft_batch)")
    outs, softs = _psk_soft_batch("d8psk", x[None, :], baud, carrier, samp_rate)
    return outs[0], softs[0]


def d8psk_demodulate_soft_batch(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000):
    """[B, N] equal-length streams -> (B bytes objects, B int8 arrays)."""
    return _psk_soft_batch("d8psk", np.asarray(samples), baud, carrier, samp_rate)


# ---------------------------------------------------------------------------
# ofdm: multi-carrier DQPSK.  K subcarriers on exact DFT bins
# of the useful part of an OFDM symbol of K * sps samples (an eighth of it the
# cyclic prefix), each carrying DQPSK across time: no filters, one dense FP64
# correlation against a twiddle table, the QPSK sync search.  Samples are
# float32, float64 or int16 PCM (read as int16 / 32768); anything else goes
# as float64.
def _ofdm_input(samples) -> np.ndarray:
    x = np.asarray(samples)
    return x if x.dtype in _amr.DTYPES else x.astype(np.float64)


def _ofdm_demod(plan, x2d, soft, acquire):
    if soft:
        outs, _, softs = plan.demod_soft_host(x2d, acquire=acquire)[:3]
        return outs, softs
    return plan.demod_host(x2d, acquire=acquire)[0], None


def _spread_demod(plan, x2d, soft, acquire):
    outs, _, softs, _ = plan.demod_host(x2d, soft=soft, acquire=acquire)
    return outs, softs


# what differs between the symbol modems (ofdm here, spread and minshift below) on the way to a plan's
# host entries: the geometry check, the plan cache's getter and the plan's demodulation as (outs, softs).
# `shape` in the functions below is ofdm's num_subcarriers / spread's code / None for minshift.
_SYM = {"ofdm": (_amr.ofdm_geometry, _amr.get_ofdm_plan, _ofdm_demod),
        "spread": (_amr.dsss_geometry, _amr.get_dsss_plan, _spread_demod),
        "minshift": (lambda baud, carrier, shape, samp_rate: _amr.msk_geometry(baud, carrier, samp_rate),
                     _amr.get_msk_plan, _spread_demod)}


def _sym_row(name: str, samples) -> np.ndarray:
    """The one stream of the 1-D entry `name` as a batch of one."""
    x = _ofdm_input(samples)
    if x.ndim != 1:
        raise ValueError(f"{name} expects a 1-D sample array (use {name}_batch)")
    return x[None, :]


def _sym_plan(modem, x2d, baud, carrier, shape, samp_rate, acquire):
    """(the batch as the kernels read it, its cached plan or None for an empty batch)"""
    x2d = _ofdm_input(x2d)
    if x2d.ndim != 2:
        raise ValueError("batch input must be a 2-D [streams, samples] array")
    B, n = x2d.shape
    _SYM[modem][0](baud, carrier, shape, samp_rate)                    # ValueError, also for an empty batch
    return x2d, (_SYM[modem][1](n, baud, carrier, shape, samp_rate, B, acquire=acquire) if B else None)


def _sym_batch(modem, x2d, baud, carrier, shape, samp_rate, soft=False, acquire=False):
    x2d, plan = _sym_plan(modem, x2d, baud, carrier, shape, samp_rate, acquire)
    if plan is None:
        return ([], []) if soft else []
    outs, softs = _SYM[modem][2](plan, x2d, soft, acquire)
    return (outs, softs) if soft else outs


def _sym_acquire(modem, x2d, baud, carrier, shape, samp_rate) -> np.ndarray:
    x2d, plan = _sym_plan(modem, x2d, baud, carrier, shape, samp_rate, True)
    return np.zeros(0, np.int64) if plan is None else plan.acquire(x2d)[0]


def ofdm_demodulate(samples, baud, carrier, num_subcarriers, samp_rate=96000, acquire=False) -> bytes:
    """Multi-carrier DQPSK demodulation of one stream, on the GPU.  acquire=True: the
    capture need not start on a symbol boundary (ofdm_acquire's offset is applied)."""
    x = _sym_row("ofdm_demodulate", samples)
    return _sym_batch("ofdm", x, baud, carrier, num_subcarriers, samp_rate, acquire=acquire)[0]


def ofdm_demodulate_batch(samples, baud, carrier, num_subcarriers, samp_rate=96000, acquire=False) -> list:
    """[B, N] equal-length streams -> B bytes objects (each == ofdm_demodulate(row))."""
    return _sym_batch("ofdm", samples, baud, carrier, num_subcarriers, samp_rate, acquire=acquire)


def ofdm_demodulate_soft(samples, baud, carrier, num_subcarriers, samp_rate=96000, acquire=False):
    """ofdm_demodulate's bytes and their soft values: (bytes, int8 array of 8 * len(bytes))."""
    x = _sym_row("ofdm_demodulate_soft", samples)
    outs, softs = _sym_batch("ofdm", x, baud, carrier, num_subcarriers, samp_rate, soft=True, acquire=acquire)
    return outs[0], softs[0]


def ofdm_demodulate_soft_batch(samples, baud, carrier, num_subcarriers, samp_rate=96000, acquire=False):
    """[B, N] equal-length streams -> (B bytes objects, B int8 arrays)."""
    return _sym_batch("ofdm", samples, baud, carrier, num_subcarriers, samp_rate, soft=True, acquire=acquire)


def ofdm_acquire_batch(samples, baud, carrier, num_subcarriers, samp_rate=96000) -> np.ndarray:
    """[B, N] equal-length streams -> int64 [B]: the sample offset o of each stream at which
    its OFDM symbols are read, in [-Ncp, L - 1 - Ncp]: the cyclic prefix's
    estimated start less half a prefix.  An aligned capture gives -(Ncp // 2).
    A symbol of fewer than 8 samples has no prefix (Ncp = L // 8 = 0): the offset is
    then 0 whatever the capture, and acquire=True decodes as acquire=False does."""
    return _sym_acquire("ofdm", samples, baud, carrier, num_subcarriers, samp_rate)


def ofdm_acquire(samples, baud, carrier, num_subcarriers, samp_rate=96000) -> int:
    """ofdm_acquire_batch of one stream."""
    return int(ofdm_acquire_batch(_sym_row("ofdm_acquire", samples), baud, carrier, num_subcarriers, samp_rate)[0])


# ---------------------------------------------------------------------------
# spread: direct-sequence DBPSK.  `baud` is the chip rate; one
# bit is a repetition of the code, despread by one FP64 correlation and decided
# differentially.  A capture may start anywhere: acquisition (the default)
# finds the code phase by a sliding code correlation over every sample offset
# of a bit.  Samples as ofdm reads them.
def spread_demodulate(samples, baud, carrier, code=None, samp_rate=96000, acquire=True) -> bytes:
    """Direct-sequence DBPSK demodulation of one stream, on the GPU.  acquire=False: the capture
    starts on a bit boundary (offset 0); the default finds the boundary first (spread_acquire)."""
    x = _sym_row("spread_demodulate", samples)
    return _sym_batch("spread", x, baud, carrier, code, samp_rate, acquire=acquire)[0]


def spread_demodulate_batch(samples, baud, carrier, code=None, samp_rate=96000, acquire=True) -> list:
    """[B, N] equal-length streams -> B bytes objects (each == spread_demodulate(row))."""
    return _sym_batch("spread", samples, baud, carrier, code, samp_rate, acquire=acquire)


def spread_demodulate_soft(samples, baud, carrier, code=None, samp_rate=96000, acquire=True):
    """spread_demodulate's bytes and their soft values: (bytes, int8 array of 8 * len(bytes))."""
    x = _sym_row("spread_demodulate_soft", samples)
    outs, softs = _sym_batch("spread", x, baud, carrier, code, samp_rate, soft=True, acquire=acquire)
    return outs[0], softs[0]


def spread_demodulate_soft_batch(samples, baud, carrier, code=None, samp_rate=96000, acquire=True):
    """[B, N] equal-length streams -> (B bytes objects, B int8 arrays)."""
    return _sym_batch("spread", samples, baud, carrier, code, samp_rate, soft=True, acquire=acquire)


def spread_acquire_batch(samples, baud, carrier, code=None, samp_rate=96000) -> np.ndarray:
    """[B, N] equal-length streams -> int64 [B]: the sample offset in [0, L - 1] at which each
    stream's bits begin: the first maximum over the offsets of a bit of the
    despread energy summed over the capture.  A bit boundary only: which bit is which is the
    sync word's business."""
    return _sym_acquire("spread", samples, baud, carrier, code, samp_rate)


def spread_acquire(samples, baud, carrier, code=None, samp_rate=96000) -> int:
    """spread_acquire_batch of one stream."""
    return int(spread_acquire_batch(_sym_row("spread_acquire", samples), baud, carrier, code, samp_rate)[0])


# ---------------------------------------------------------------------------
# minshift: MSK, continuous phase and constant envelope, the two
# tones half the bit rate apart.  One FP64 correlation per bit boundary, decided
# differentially.  A capture may start anywhere: the bit timing (the default) is
# read from the two spectral lines of the squared signal, with no search.
# Samples as ofdm reads them.
def minshift_demodulate(samples, baud, carrier, samp_rate=96000, acquire=True) -> bytes:
    """MSK demodulation of one stream, on the GPU.  acquire=False: the capture starts on a
    bit boundary (offset 0); the default finds the bit timing first (minshift_acquire)."""
    x = _sym_row("minshift_demodulate", samples)
    return _sym_batch("minshift", x, baud, carrier, None, samp_rate, acquire=acquire)[0]


def minshift_demodulate_batch(samples, baud, carrier, samp_rate=96000, acquire=True) -> list:
    """[B, N] equal-length streams -> B bytes objects (each == minshift_demodulate(row))."""
    return _sym_batch("minshift", samples, baud, carrier, None, samp_rate, acquire=acquire)


def minshift_demodulate_soft(samples, baud, carrier, samp_rate=96000, acquire=True):
    """minshift_demodulate's bytes and their soft values: (bytes, int8 array of 8 * len(bytes))."""
    x = _sym_row("minshift_demodulate_soft", samples)
    outs, softs = _sym_batch("minshift", x, baud, carrier, None, samp_rate, soft=True, acquire=acquire)
    return outs[0], softs[0]


def minshift_demodulate_soft_batch(samples, baud, carrier, samp_rate=96000, acquire=True):
    """[B, N] equal-length streams -> (B bytes objects, B int8 arrays)."""
    return _sym_batch("minshift", samples, baud, carrier, None, samp_rate, soft=True, acquire=acquire)


def minshift_acquire_batch(samples, baud, carrier, samp_rate=96000) -> np.ndarray:
    """[B, N] equal-length streams -> int64 [B]: the sample offset in [0, L - 1] at which each
    stream's bits begin, from the phase difference of the squared signal's two
    spectral lines.  One offset per capture, on the sender's sample clock; a bit boundary
    only: which bit is which is the sync word's business."""
    return _sym_acquire("minshift", samples, baud, carrier, None, samp_rate)


def minshift_acquire(samples, baud, carrier, samp_rate=96000) -> int:
    """minshift_acquire_batch of one stream."""
    return int(minshift_acquire_batch(_sym_row("minshift_acquire", samples), baud, carrier, samp_rate)[0])


# ---------------------------------------------------------------------------
# tone8: 8-FSK with Costas sync, continuous phase and constant
# envelope, eight orthogonal tones one symbol rate apart, three bits per symbol,
# nothing differential.  A capture may start anywhere and its sender may sit up
# to `search` half tone spacings off the receiver's carrier: acquisition (the
# default) finds both with one 2-D correlation of the 7x7 Costas block over the
# capture's spectrogram.  Samples as ofdm reads them.
def _tone8_demod(plan, x2d, soft, acquire):
    outs, _, softs, _, _ = plan.demod_host(x2d, soft=soft, acquire=acquire)
    return outs, softs


_SYM["tone8"] = (lambda baud, carrier, shape, samp_rate: _amr.tone8_geometry(baud, carrier, samp_rate, shape),
                 _amr.get_tone8_plan, _tone8_demod)


def tone8_demodulate(samples, baud, carrier, samp_rate=96000, acquire=True, search=6) -> bytes:
    """8-FSK demodulation of one stream, on the GPU.  acquire=False: the capture starts on a symbol
    boundary and its tones sit on the receiver's (`search` is not used); the default finds both first
    (tone8_acquire), which needs carrier / baud >= 1 + search / 4."""
    x = _sym_row("tone8_demodulate", samples)
    return _sym_batch("tone8", x, baud, carrier, search if acquire else 0, samp_rate, acquire=acquire)[0]


def tone8_demodulate_batch(samples, baud, carrier, samp_rate=96000, acquire=True, search=6) -> list:
    """[B, N] equal-length streams -> B bytes objects (each == tone8_demodulate(row))."""
    return _sym_batch("tone8", samples, baud, carrier, search if acquire else 0, samp_rate, acquire=acquire)


def tone8_demodulate_soft(samples, baud, carrier, samp_rate=96000, acquire=True, search=6):
    """tone8_demodulate's bytes and their soft values: (bytes, int8 array of 8 * len(bytes))."""
    x = _sym_row("tone8_demodulate_soft", samples)
    outs, softs = _sym_batch("tone8", x, baud, carrier, search if acquire else 0, samp_rate, soft=True, acquire=acquire)
    return outs[0], softs[0]


def tone8_demodulate_soft_batch(samples, baud, carrier, samp_rate=96000, acquire=True, search=6):
    """[B, N] equal-length streams -> (B bytes objects, B int8 arrays)."""
    return _sym_batch("tone8", samples, baud, carrier, search if acquire else 0, samp_rate, soft=True, acquire=acquire)


def tone8_acquire_batch(samples, baud, carrier, samp_rate=96000, search=6):
    """[B, N] equal-length streams -> (start int64 [B], shift int64 [B]): the sample at
    which each stream's Costas block begins, on a grid of L // 8 samples, and how far the sender's tones
    are from the receiver's in half tone spacings (baud / 2 Hz each), -search .. search.  One pair per
    capture, on the sender's sample clock; neither is refined, and there is no confidence value."""
    x2d, plan = _sym_plan("tone8", samples, baud, carrier, search, samp_rate, True)
    if plan is None:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return plan.acquire(x2d)[:2]


def tone8_acquire(samples, baud, carrier, samp_rate=96000, search=6):
    """tone8_acquire_batch of one stream: (start, shift)."""
    start, shift = tone8_acquire_batch(_sym_row("tone8_acquire", samples), baud, carrier, samp_rate, search)
    return int(start[0]), int(shift[0])


# ---------------------------------------------------------------------------
# star16: two-ring 16-ary differential amplitude and phase keying (DESIGN.md
# §3o).  QPSK's front end, d8psk's tribit on the differential product and a
# ring bit from the two symbols' energies; differential in both, so it needs no
# gain control and no carrier phase reference.
def star16_demodulate(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000) -> bytes:
    """Two-ring 16-DAPSK demodulation of one stream, on the GPU."""
    x = _as_batch(samples)
    if x.ndim != 1:
        raise ValueError("star16_demodulate expects a 1-D sample array (use star16_demodulate_batch)")
    return _psk_batch("star16", x[None, :], baud, carrier, samp_rate)[0]


def star16_demodulate_batch(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000) -> list:
    """[B, N] equal-length streams -> B bytes objects (each == star16_demodulate(row))."""
    return _psk_batch("star16", np.asarray(samples), baud, carrier, samp_rate)


def star16_demodulate_soft(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000):
    """star16_demodulate's bytes and their soft values: (bytes, int8 array of 8 * len(bytes)).
    Four values per symbol, a, b2, b1, b0; a's magnitude is 64 at equal energies
    and 51 at a clean ring change, b0's tops out near 74 as d8psk's."""
    x = _as_batch(samples)
    if x.ndim != 1:
        raise ValueError("star16_demodulate_soft expects a 1-D sample array (use star16_demodulate_soft_batch)")
    outs, softs = _psk_soft_batch("star16", x[None, :], baud, carrier, samp_rate)
    return outs[0], softs[0]


def star16_demodulate_soft_batch(samples: np.ndarray, baud=1200, carrier=3000.0, samp_rate=96000):
    """[B, N] equal-length streams -> (B bytes objects, B int8 arrays)."""
    return _psk_soft_batch("star16", np.asarray(samples), baud, carrier, samp_rate)


def _pcm16_star16(pcm: np.ndarray, baud, carrier=3000.0, samp_rate=96000) -> bytes:
    """16-bit WAV samples as pcm / 32768 (as _pcm16_psk): star16_demodulate of that capture."""
    return _pcm16_psk("star16", pcm, baud, carrier, samp_rate)


def demodulate_ragged(kind: str, streams, baud, carrier=3000.0, samp_rate=96000) -> list:
    """Ragged batch: streams of different lengths and dtypes, grouped by
    (length, dtype) on the host -- each result == <kind>_demodulate(stream):
    a stream keeps its own dtype (and with it its odd extension, _as_batch)
    rather than the one numpy would promote a mixed stack to."""
    fn = {"qpsk": qpsk_demodulate_batch, "bpsk": bpsk_demodulate_batch, "d8psk": d8psk_demodulate_batch,
          "star16": star16_demodulate_batch}[kind]
    rows = [_as_batch(s) for s in streams]
    groups: dict = {}
    for i, r in enumerate(rows):
        groups.setdefault((len(r), r.dtype), []).append(i)
    out = [b""] * len(streams)
    for idx in groups.values():
        res = fn(np.stack([rows[i] for i in idx]), baud, carrier, samp_rate)
        for i, r in zip(idx, res):
            out[i] = r
    return out


# ---------------------------------------------------------------------------
# FSK receive side (modem.py:298-341): tone band-passes + |hilbert| envelopes
def fsk_demodulate(samples: np.ndarray, baud=1200, mark_freq=1200.0, space_freq=2200.0, samp_rate=96000) -> bytes:
    x = _as_batch(samples)
    if x.ndim != 1:
        raise ValueError("fsk_demodulate expects a 1-D sample array (use fsk_demodulate_batch)")
    return fsk_demodulate_batch(x[None, :], baud, mark_freq, space_freq, samp_rate)[0]


def fsk_demodulate_batch(samples: np.ndarray, baud=1200, mark_freq=1200.0, space_freq=2200.0,
                         samp_rate=96000) -> list:
    import _fsk
    return _fsk.fsk_demodulate_batch(_as_batch(np.asarray(samples)), baud, mark_freq, space_freq, samp_rate, raw=True)


# ---------------------------------------------------------------------------
# aliases kept from the reference (modem.py:344-403)
def psk8_modulate(d, b=1200, c=3000.0, s=96000):
    return qpsk_modulate(d, b, c, s)


def psk8_demodulate(s, b=1200, c=3000.0, s_r=96000):
    return qpsk_demodulate(s, b, c, s_r)


def fsk_high_speed_modulate(d, baud=19200, s=96000):
    return fsk_modulate(d, baud, 8000, 16000, s)


def fsk_high_speed_demodulate(s, baud=19200, s_r=96000):
    return fsk_demodulate(s, baud, 8000, 16000, s_r)


def ofdm_modulate_simple(d, baud, carrier, num_subcarriers, samp_rate=96000):
    return qpsk_modulate(d, baud, carrier, samp_rate)


def ofdm_demodulate_simple(s, baud, carrier, num_subcarriers, samp_rate=96000):
    return qpsk_demodulate(s, baud, carrier, samp_rate)


def apsk16_modulate(d, b, c, s=96000):
    return qpsk_modulate(d, b, c, s)


def dsss_modulate(d, b, c, s=96000):
    return bpsk_modulate(d, b, c, s)


def msk_modulate(d, b, c, s=96000):
    return fsk_modulate(d, b, c, c + b, s)


def ft8_modulate(d, b, c, s=96000):
    return fsk_modulate(d, 50, c, c + 50, s)


def ft8_demodulate(s, b, c, sr=96000):
    return fsk_demodulate(s, 50, c, c + 50, sr)


def psk31_modulate(d, b, c, s=96000):
    return bpsk_modulate(d, 31.25, c, s)


def psk31_demodulate(s, b, c, sr=96000):
    return bpsk_demodulate(s, 31.25, c, sr)


# ---------------------------------------------------------------------------
# Hellschreiber (hellschreiber.py; modem.py:400-403): a per-pixel energy
# detector + 7-pixel glyph lookup on receive (hell_kernels.hip, numpy's own
# summation order and dtypes, so the decisions are np.mean(chunk ** 2) > 0.1's
# bit for bit), on/off keyed glyph pixels on transmit (tx_kernels.hip).
def _hell_sps(baud, samp_rate, tx=False) -> int:
    """hellschreiber.py:135, 158 -- with Python's own exceptions for a zero /
    non-finite baud (ZeroDivisionError, OverflowError, ValueError); tx: also
    numpy's ValueError for a waveform of <= 0 samples per pixel (host
    arithmetic in libamr.so, before any device work)."""
    sps = int(round(samp_rate / baud))
    if tx:
        _amr.tx_samples(_amr.TX_HELL, 0, baud, samp_rate)
    return sps


def hellschreiber_modulate(text: str, baud=122.5, carrier=1000.0, samp_rate=SAMPLE_RATE) -> np.ndarray:
    """hellschreiber.py:109-152: 70 sync pixels, per character 7 x 7 glyph bits +
    2 blank (51 blank for a character outside the map), 35 end pixels; each
    on-pixel a carrier burst, the whole normalised to 0.8."""
    _hell_sps(baud, samp_rate, tx=True)
    return _amr.modulate(_amr.TX_HELL, [_amr.hell_payload(text)], baud, carrier, 0.0, samp_rate)[0]


def feld_hell_modulate(d, b, c, s=96000):
    return hellschreiber_modulate(d.decode('utf-8', 'ignore'), b, c, s)


def _hell_batch(x2d: np.ndarray, baud, samp_rate, elem=None) -> list:
    if x2d.ndim != 2:
        raise ValueError("batch input must be a 2-D [streams, samples] array")
    elem = _amr.hell_elem(x2d.dtype) if elem is None else elem      # TypeError names an unsupported dtype
    if _hell_sps(baud, samp_rate) < 0 and x2d.shape[0] > 0:         # range() with a negative step: nothing decoded
        return [b""] * x2d.shape[0]
    return _amr.hell_demod(x2d, baud, samp_rate, elem)


def feld_hell_demodulate(s, b, c, sr=96000):
    """hellschreiber_demodulate(s, b, c, sr).encode('utf-8') (modem.py:403;
    the carrier is unused there too), on the GPU."""
    x = np.asarray(s)
    if x.ndim != 1:
        raise ValueError("feld_hell_demodulate expects a 1-D sample array (use feld_hell_demodulate_batch)")
    return _hell_batch(x[None, :], b, sr)[0]


def feld_hell_demodulate_batch(samples: np.ndarray, baud=122.5, carrier=1000.0, samp_rate=96000) -> list:
    """[B, N] equal-length captures -> B bytes objects (each == feld_hell_demodulate(row))."""
    return _hell_batch(np.asarray(samples), baud, samp_rate)


def _pcm16_hell(pcm: np.ndarray, baud=122.5, carrier=1000.0, samp_rate=96000) -> bytes:
    """16-bit WAV samples as pcm / 32768 in float64 (decoder._Pcm16), converted on the device."""
    x = np.ascontiguousarray(pcm, np.int16)[None, :]
    return _hell_batch(x, baud, samp_rate, elem=_amr.HELL_PCM16)[0]


# ---------------------------------------------------------------------------
# transmit side on the GPU (tx_kernels.hip): the same float32
# samples as the reference's modulators; wav_from_array stays a host WAV writer.
def bpsk_modulate(data_bytes: bytes, baud=1200, carrier=3000.0, samp_rate=96000) -> np.ndarray:
    """modem.py:28-65 (DBPSK)."""
    return _amr.modulate(_amr.TX_BPSK, [bytes(data_bytes)], baud, carrier, 0.0, samp_rate)[0]


def qpsk_modulate(data_bytes: bytes, baud=1200, carrier=3000.0, samp_rate=96000) -> np.ndarray:
    """modem.py:138-186 (DQPSK)."""
    return _amr.modulate(_amr.TX_QPSK, [bytes(data_bytes)], baud, carrier, 0.0, samp_rate)[0]


def fsk_modulate(data_bytes: bytes, baud=1200, mark_freq=1200.0, space_freq=2200.0, samp_rate=96000) -> np.ndarray:
    """modem.py:270-295 (CPFSK)."""
    return _amr.modulate(_amr.TX_FSK, [bytes(data_bytes)], baud, mark_freq, space_freq, samp_rate)[0]


def d8psk_modulate(data_bytes: bytes, baud=1200, carrier=3000.0, samp_rate=96000) -> np.ndarray:
    """8-ary differential PSK: [0,0,0]*30 + [1,1,0]*10 + the payload's
    bits, three per symbol as a Gray-coded phase step of k * pi/4, on a
    phase-continuous carrier; 40 + ceil(8 len / 3) symbols."""
    return _amr.modulate(_amr.TX_D8PSK, [bytes(data_bytes)], baud, carrier, 0.0, samp_rate)[0]


def star16_modulate(data_bytes: bytes, baud=1200, carrier=3000.0, samp_rate=96000) -> np.ndarray:
    """Two-ring 16-DAPSK: [0,0,0,0]*30 + [1,1,1,0]*10 + the payload's bits, four
    per symbol: a ring toggle (amplitude 1.0 / 0.5) and d8psk's Gray-coded phase step, on a
    phase-continuous carrier under a parabolic symbol envelope; 40 + 2 len symbols."""
    return _amr.modulate(_amr.TX_STAR16, [bytes(data_bytes)], baud, carrier, 0.0, samp_rate)[0]


def ofdm_modulate(data_bytes: bytes, baud, carrier, num_subcarriers, samp_rate=96000) -> np.ndarray:
    """Multi-carrier DQPSK: [0,0]*30 + [1,1]*10 + the payload's bits,
    zero-padded to a multiple of 2 K; dibit j on OFDM symbol 1 + j // K, subcarrier
    j % K, as a phase step from the symbol before; symbol 0 carries the Newman
    reference phases.  (1 + ceil((40 + 4 len) / K)) * K * sps samples."""
    return _amr.ofdm_modulate([bytes(data_bytes)], baud, carrier, num_subcarriers, samp_rate)[0]


def spread_modulate(data_bytes: bytes, baud, carrier, code=None, samp_rate=96000) -> np.ndarray:
    """Direct-sequence DBPSK: [1,0]*40 + the payload's bits, one bit per
    repetition of `code` (default _amr.DSSS_CODE, 16 chips) at `baud` chips per second, a 1 as a
    sign change from the bit before; a bit holds a whole number of carrier cycles, so the
    carrier is continuous.  (81 + 8 len) * C * spc samples."""
    return _amr.dsss_modulate([bytes(data_bytes)], baud, carrier, code, samp_rate)[0]


def minshift_modulate(data_bytes: bytes, baud, carrier, samp_rate=96000) -> np.ndarray:
    """MSK: [0] + [1,0]*40 + the payload's bits + [0], a 1 as cyc4 + 1 and a 0
    as cyc4 - 1 quarter-cycles of phase over the bit, the phase continuous and the envelope
    constant; the tones are half the bit rate apart.  (82 + 8 len) * L samples."""
    return _amr.msk_modulate([bytes(data_bytes)], baud, carrier, samp_rate)[0]


def tone8_modulate(data_bytes: bytes, baud, carrier, samp_rate=96000) -> np.ndarray:
    """8-FSK with Costas sync: the Costas block 3, 1, 4, 0, 6, 5, 2, then the payload's
    bits three per symbol (MSB first, zero-padded), tribit v on tone v ^ (v >> 1); tone m has c2 + 2 m
    half-cycles per symbol, the phase continuous and the envelope constant.  (7 + ceil(8 len / 3)) * L
    samples."""
    return _amr.tone8_modulate([bytes(data_bytes)], baud, carrier, samp_rate)[0]


def modulate_batch(kind: str, datas, baud=1200, f0=None, f1=None, samp_rate=96000, n_out=None, pcm=False,
                   num_subcarriers=None, code=None):
    """Batched modulators: [B, n_out] float32 (each row == <kind>_modulate(datas[b])
    cut / zero-padded to n_out; default the longest), plus wav_from_array's
    int16 samples when pcm=True.  kind: 'bpsk' | 'qpsk' | 'd8psk' | 'star16' (f0 = carrier) or
    'fsk' (f0 = mark_freq, f1 = space_freq), or 'hell' (datas: texts or UTF-8
    bytes, decoded as feld_hell_modulate does; f0 = carrier, default 1000;
    pass baud=122.5 for the reference's default), or 'ofdm' (f0 = carrier,
    num_subcarriers required), or 'spread' (f0 = carrier, baud = the chip rate,
    code: the chips, default _amr.DSSS_CODE), or 'minshift' or 'tone8' (f0 = carrier)."""
    if kind == "tone8":
        return _amr.tone8_modulate([bytes(d) for d in datas], baud, 3000.0 if f0 is None else f0, samp_rate, n_out, pcm)
    if kind == "minshift":
        return _amr.msk_modulate([bytes(d) for d in datas], baud, 3000.0 if f0 is None else f0, samp_rate, n_out, pcm)
    if kind == "spread":
        return _amr.dsss_modulate([bytes(d) for d in datas], baud, 3000.0 if f0 is None else f0, code, samp_rate,
                                  n_out, pcm)
    if kind == "ofdm":
        if num_subcarriers is None:
            raise ValueError("modulate_batch('ofdm', ...) needs num_subcarriers")
        return _amr.ofdm_modulate([bytes(d) for d in datas], baud, 3000.0 if f0 is None else f0, num_subcarriers,
                                  samp_rate, n_out, pcm)
    mode = _amr.TX_MODES[kind]
    if kind == "hell":
        _hell_sps(baud, samp_rate, tx=True)
        texts = [d if isinstance(d, str) else bytes(d).decode('utf-8', 'ignore') for d in datas]
        return _amr.modulate(mode, [_amr.hell_payload(t) for t in texts], baud, 1000.0 if f0 is None else f0, 0.0,
                             samp_rate, n_out, pcm)
    if f0 is None:
        f0 = 1200.0 if kind == "fsk" else 3000.0
    if f1 is None:
        f1 = 2200.0 if kind == "fsk" else 0.0
    return _amr.modulate(mode, [bytes(d) for d in datas], baud, f0, f1, samp_rate, n_out, pcm)


def wav_from_array(arr, sr=96000):
    """modem.py:360-368: 16-bit mono WAV of int16(arr * 32767)."""
    return synth.wav_bytes(arr, sr)
