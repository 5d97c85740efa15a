"""ctypes binding of libamr.so (include/amr.h) + the host-side plan cache.

This is the thin host layer between the reference-shaped Python API
(modem.py / decoder.py / fec.py in this directory) and the HIP kernels.
There is deliberately NO CPU fallback: if libamr.so is missing or no GPU is
visible, every demodulation raises AmrError.

Filter design happens here, on the host, with the same scipy calls the
reference makes (modem.py:73-76/86-87 BPSK, modem.py:194-197/203 QPSK), so the
coefficients -- and scipy's ValueError messages -- are the reference's own.
"""
from __future__ import annotations

import ctypes
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AMR_LIB", os.path.join(HERE, "libamr.so"))

AMR_OK = 0
AMR_E_INVALID, AMR_E_PADLEN, AMR_E_HIP, AMR_E_NOMEM, AMR_E_NODEVICE, AMR_E_RCCL, AMR_E_CAPACITY = \
    -1, -2, -3, -4, -5, -6, -7
DTYPE_F32, DTYPE_F64, DTYPE_I16 = 0, 1, 2
PSK_QPSK, PSK_BPSK, PSK_D8PSK = 0, 1, 2
# a demodulator's kind name -> AMR_PSK_* and its bits per symbol; "d8psk" (the
# 8-ary differential modem) has QPSK's design (design_psk)
PSK_KINDS = {"qpsk": PSK_QPSK, "bpsk": PSK_BPSK, "d8psk": PSK_D8PSK}
PSK_BITS = {"qpsk": 2, "bpsk": 1, "d8psk": 3}
# the later kinds: "star16" (the two-ring 16-DAPSK modem; QPSK's
# design too).  The host layer looks a kind up through psk_kind / psk_bits,
# which know these and the three above
PSK_STAR16 = 4
PSK_KINDS_MORE = {"star16": PSK_STAR16}
PSK_BITS_MORE = {"star16": 4}


def psk_kind(kind: str) -> int:
    """AMR_PSK_* of a demodulator's kind name (KeyError names an unknown one)."""
    return PSK_KINDS_MORE[kind] if kind in PSK_KINDS_MORE else PSK_KINDS[kind]


def psk_bits(kind: str) -> int:
    """Bits per symbol of a demodulator's kind name."""
    return PSK_BITS_MORE[kind] if kind in PSK_BITS_MORE else PSK_BITS[kind]


T_NAMES = ["bandpass", "lowpass_fwd", "lowpass_bwd", "lowpass_exact", "sync_pack", "fec", "launch"]
TF_NAMES = ["bandpass", "hilbert", "decide", "launch", "exact"]
# amr_frame_rec (include/amr.h), 64 bytes
FRAME_SHORT, FRAME_NONAME, FRAME_NOMETA, FRAME_BADLEN, FRAME_INCOMPLETE, FRAME_CRC_BAD, FRAME_OK = range(7)
FRAME_REC = np.dtype([("start", "<i8"), ("name_start", "<i8"), ("payload_start", "<i8"), ("status", "<i4"),
                      ("name_len", "<i4"), ("part", "<u4"), ("total", "<u4"), ("fsize", "<u4"), ("fcrc", "<u4"),
                      ("dlen", "<u4"), ("pcrc", "<u4"), ("calc_crc", "<u4"), ("reserved", "<u4")])
assert FRAME_REC.itemsize == 64
DTYPES = {np.dtype(np.float32): DTYPE_F32, np.dtype(np.float64): DTYPE_F64, np.dtype(np.int16): DTYPE_I16}

# every symbol include/amr.h declares (tests/test_abi.py checks the export table)
EXPORTS = [
    "amr_abi_version", "amr_build_id", "amr_last_error", "amr_device_count", "amr_set_device", "amr_malloc", "amr_free",
    "amr_memcpy_h2d", "amr_memcpy_d2h", "amr_memcpy_d2d", "amr_device_synchronize",
    "amr_psk_plan_create", "amr_psk_plan_destroy", "amr_psk_plan_out_capacity", "amr_psk_plan_scratch_bytes",
    "amr_psk_plan_bytes_estimate", "amr_fsk_plan_bytes_estimate",
    "amr_psk_plan_synchronize", "amr_psk_plan_enable_timing", "amr_psk_plan_timings", "amr_psk_plan_set_inflight",
    "amr_psk_plan_exact_streams", "amr_psk_demod_host", "amr_psk_demod_device", "amr_psk_demod_fec_device",
    "amr_psk_slice_host", "amr_sync_pack_host", "amr_psk_plan_last_layout", "amr_synth_tile_noise",
    "amr_psk_demod_host_async", "amr_fsk_demod_host_async", "amr_host_register", "amr_host_unregister",
    "amr_host_alloc", "amr_host_free",
    "amr_fsk_plan_create", "amr_fsk_plan_destroy", "amr_fsk_plan_out_capacity", "amr_fsk_plan_scratch_bytes",
    "amr_fsk_plan_resident_bytes",
    "amr_fsk_plan_fft_length", "amr_fsk_plan_live_columns", "amr_fsk_plan_synchronize", "amr_fsk_plan_enable_timing", "amr_fsk_plan_timings",
    "amr_fsk_demod_host", "amr_fsk_demod_device", "amr_fsk_envelopes_host", "amr_fft_c2c_host", "amr_hilbert_host",
    "amr_fec_decode_host", "amr_frame_parse_host", "amr_frame_parse_device", "amr_comm_unique_id", "amr_comm_create", "amr_comm_destroy", "amr_allgather", "amr_fsk_allgather",
    "amr_comm_synchronize", "amr_comm_allgather_host", "amr_comm_allreduce_max", "amr_comm_world", "amr_tx_samples", "amr_tx_work_bytes", "amr_modulate_host", "amr_modulate_device",
    "amr_resample_host", "amr_hilbert_env_exact_host", "amr_fsk_plan_exact_streams",
    "amr_fsk_plan_set_exact_mode", "amr_psk_plan_set_layout", "amr_psk_plan_split_info", "amr_psk_split_design",
    "amr_psk_split_symbols_host", "amr_psk_f32_margin", "amr_psk_plan_last_f32f", "amr_psk_plan_last_lowpass", "amr_split_state_tables",
    "amr_psk_plan_split_conv",
    "amr_fsk_plan_set_layout", "amr_fsk_plan_split_info", "amr_fsk_split_design", "amr_fsk_split_bandpass_host",
    "amr_fsk_fft_margin", "amr_fsk_plan_margin", "amr_fsk_plan_set_split_strict", "amr_fsk_plan_split_strict",
    "amr_fsk_plan_last_strict", "amr_fsk_split_strict_design", "amr_fsk_split_bounds_host",
    "amr_fsk_plan_split_conv",
    "amr_psk_demod_host_edges", "amr_psk_demod_device_edges", "amr_fsk_demod_host_edges", "amr_fsk_demod_device_edges",
    "amr_psk_split_bounds_host", "amr_psk_plan_set_split_strict", "amr_psk_plan_split_strict",
    "amr_psk_plan_last_strict", "amr_psk_split_strict_design",
    "amr_hell_pixels", "amr_hell_work_bytes", "amr_hell_demod_host", "amr_hell_demod_device", "amr_hell_glyph_rows",
    "amr_conv_encoded_len", "amr_conv_encode_host", "amr_viterbi_work_bytes", "amr_viterbi_decode_device",
    "amr_viterbi_decode_host",
    "amr_psk_demod_soft_host", "amr_psk_demod_soft_device", "amr_psk_soft_host", "amr_viterbi_soft_work_bytes",
    "amr_viterbi_decode_soft_device", "amr_viterbi_decode_soft_host",
    "amr_rs_encoded_len", "amr_rs_decoded_len", "amr_rs_encode_host", "amr_rs_encode_device", "amr_rs_decode_host",
    "amr_rs_decode_device",
    "amr_ofdm_plan_create", "amr_ofdm_plan_destroy", "amr_ofdm_plan_synchronize", "amr_ofdm_plan_enable_timing",
    "amr_ofdm_plan_timings", "amr_ofdm_plan_out_capacity", "amr_ofdm_plan_scratch_bytes",
    "amr_ofdm_plan_bytes_estimate", "amr_ofdm_demod_host", "amr_ofdm_demod_device", "amr_ofdm_demod_soft_host",
    "amr_ofdm_demod_soft_device", "amr_ofdm_symbols_host", "amr_ofdm_slice_host", "amr_ofdm_soft_host",
    "amr_ofdm_modulate_host", "amr_ofdm_acquire_bytes_estimate", "amr_ofdm_acquire_host", "amr_ofdm_acquire_device",
    "amr_ofdm_symbols_at_host", "amr_ofdm_demod_acq_host", "amr_ofdm_demod_acq_device",
    "amr_dsss_plan_create", "amr_dsss_plan_destroy", "amr_dsss_plan_synchronize", "amr_dsss_plan_enable_timing",
    "amr_dsss_plan_timings", "amr_dsss_plan_out_capacity", "amr_dsss_plan_scratch_bytes",
    "amr_dsss_plan_bytes_estimate", "amr_dsss_acquire_bytes_estimate", "amr_dsss_demod_host", "amr_dsss_demod_device",
    "amr_dsss_acquire_host", "amr_dsss_acquire_device", "amr_dsss_symbols_at_host", "amr_dsss_slice_host",
    "amr_dsss_soft_host", "amr_dsss_modulate_host",
    "amr_msk_plan_create", "amr_msk_plan_destroy", "amr_msk_plan_synchronize", "amr_msk_plan_enable_timing",
    "amr_msk_plan_timings", "amr_msk_plan_out_capacity", "amr_msk_plan_scratch_bytes",
    "amr_msk_plan_bytes_estimate", "amr_msk_acquire_bytes_estimate", "amr_msk_demod_host", "amr_msk_demod_device",
    "amr_msk_acquire_host", "amr_msk_acquire_device", "amr_msk_symbols_at_host", "amr_msk_offset_host",
    "amr_msk_slice_host", "amr_msk_soft_host", "amr_msk_modulate_host",
    "amr_tone8_chunk", "amr_tone8_plan_create", "amr_tone8_plan_destroy", "amr_tone8_plan_synchronize",
    "amr_tone8_plan_enable_timing", "amr_tone8_plan_timings", "amr_tone8_plan_out_capacity",
    "amr_tone8_plan_scratch_bytes", "amr_tone8_plan_bytes_estimate", "amr_tone8_acquire_bytes_estimate",
    "amr_tone8_demod_host", "amr_tone8_demod_device", "amr_tone8_acquire_host", "amr_tone8_acquire_device",
    "amr_tone8_symbols_at_host", "amr_tone8_peak_host", "amr_tone8_slice_host", "amr_tone8_soft_host",
    "amr_tone8_modulate_host",
]
TO_NAMES = ["dft", "slice", "sync_pack", "launch"]
TO_SLOTS = TO_NAMES + ["acquire"]                  # AMR_TO_*: "acquire" is run by an acquiring call only
OFDM_MAX_K = 64
TD_SLOTS = ["despread", "slice", "sync_pack", "launch", "acquire"]   # AMR_TD_*: "acquire" on acquiring calls only
DSSS_MAX_C = 64
# spread's default code, 0x8B63: balanced, no cyclic run longer than 3, every off-peak
# even and odd periodic autocorrelation within 4 of 16
DSSS_CODE = [1, 0, 0, 0, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0, 1, 1]

TX_BPSK, TX_QPSK, TX_FSK, TX_HELL, TX_D8PSK, TX_STAR16 = 0, 1, 2, 3, 4, 6
TX_MODES = {"bpsk": TX_BPSK, "qpsk": TX_QPSK, "fsk": TX_FSK, "hell": TX_HELL, "d8psk": TX_D8PSK,
            "star16": TX_STAR16}

# AMR_HELL_ELEM_* (include/amr.h): the element types the Hellschreiber receiver reads
HELL_PCM16 = 11
HELL_ELEMS = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.float16): 2,
              np.dtype(np.int8): 3, np.dtype(np.int16): 4, np.dtype(np.int32): 5, np.dtype(np.int64): 6,
              np.dtype(np.uint8): 7, np.dtype(np.uint16): 8, np.dtype(np.uint32): 9, np.dtype(np.uint64): 10}
HELL_BLANK = 255                                       # payload index of a character outside the glyph table


def tx_samples(mode: int, n_bytes: int, baud, samp_rate) -> int:
    """len() of the reference modulator's output for an n_bytes payload."""
    n = lib().amr_tx_samples(mode, n_bytes, float(baud), float(samp_rate))
    if n < 0:
        _raise_tx(int(n))
    return int(n)


def _raise_tx(rc: int):
    msg = lib().amr_last_error().decode("utf-8", "replace")
    if msg.startswith("could not broadcast"):
        raise ValueError(msg)                      # numpy's error, modem.py:58-61 / 181-183
    if msg == "float division by zero":
        raise ZeroDivisionError(msg)
    if msg.startswith(("zero-size array", "negative dimensions", "range() arg 3")):
        raise ValueError(msg)                      # numpy's / range()'s error, hellschreiber.py:137, 148, 162
    raise AmrError(rc, msg)


def hell_glyph_rows() -> np.ndarray:
    """The glyph bitmaps libamr.so carries: [95][7] uint8 for ' '..'~' (byte r =
    pixel row r, bit i = the row's i-th pixel on the air).  Host only."""
    rows = np.zeros((95, 7), np.uint8)
    lib().amr_hell_glyph_rows(ptr(rows), None)
    return rows


def hell_rx_lookup() -> bytes:
    """The receiver's 128-entry lookup (7-pixel value -> character).  Host only."""
    lut = np.zeros(128, np.uint8)
    lib().amr_hell_glyph_rows(None, ptr(lut))
    return lut.tobytes()


def hell_payload(text: str) -> bytes:
    """One glyph index per character of `text` (AMR_TX_HELL's payload)."""
    return bytes(ord(c) - 0x20 if 0x20 <= ord(c) <= 0x7E else HELL_BLANK for c in text)


def hell_elem(dtype) -> int:
    """AMR_HELL_ELEM_* for a raw capture's dtype; TypeError (naming it) for one
    numpy's arithmetic cannot be restated for (longdouble, complex, object ...)."""
    dt = np.dtype(dtype)
    if dt.kind == "b":
        dt = np.dtype(np.int8)                         # bool ** 2 is int8
    e = HELL_ELEMS.get(dt.newbyteorder("=") if dt.kind in "iuf" else dt)
    if e is None:
        raise TypeError(f"feld_hell_demodulate: unsupported sample dtype {np.dtype(dtype)}")
    return e


def hell_demod(x: np.ndarray, baud, samp_rate, elem=None, energy=False):
    """hellschreiber_demodulate of every row of x [B][N] on the GPU
    (amr_hell_demod_host): list of bytes; with energy=True also the pixels'
    np.mean(chunk ** 2) values [B][pixels] widened to float64.  elem: an
    AMR_HELL_ELEM_* override (HELL_PCM16 for int16 PCM); default from x.dtype."""
    if elem is None:
        elem = hell_elem(x.dtype)
    if x.dtype.kind == "b":
        x = x.astype(np.int8)
    if not x.dtype.isnative:
        x = x.astype(x.dtype.newbyteorder("="))
    if x.ndim != 2:
        raise ValueError("batch input must be a 2-D [streams, samples] array")
    B, n = x.shape
    if x.strides[1] != x.itemsize or (B > 1 and (x.strides[0] % x.itemsize or x.strides[0] < n * x.itemsize)):
        x = np.ascontiguousarray(x)                    # rows of a wider array go as they are (x_stride)
    stride = x.strides[0] // x.itemsize if B > 1 else n
    n_pix = int(lib().amr_hell_pixels(n, float(baud), float(samp_rate)))
    if n_pix < 0:
        _raise_tx(n_pix)
    if B == 0:
        return ([], np.zeros((0, n_pix))) if energy else []
    require_gpu()
    check(lib().amr_set_device(default_device()))
    cap = max(1, n_pix // 7)
    out = np.zeros((B, cap), np.uint8)
    ln = np.zeros(B, np.int64)
    en = np.zeros((B, n_pix), np.float64) if energy else None
    rc = lib().amr_hell_demod_host(ptr(x), int(elem), B, stride, n, float(baud), float(samp_rate), ptr(out), cap, ptr(ln), ptr(en) if energy else None)
    if rc != AMR_OK:
        _raise_tx(rc)
    outs = [out[i, :ln[i]].tobytes() for i in range(B)]
    return (outs, en) if energy else outs


def _modulate_call(datas, n_out, pcm, call):
    """The *_modulate_host entries' common arguments: the payloads packed into [n][stride] uint8 with their
    lengths, out [n][n_out] float32 and, with pcm, int16.  call(data, data_stride, n_bytes, n, out,
    out_stride, n_out, pcm, pcm_stride) -> rc; returns (rc, out or (out, pcm))."""
    n = len(datas)
    lens = np.array([len(d) for d in datas], np.int64)
    stride = max(1, int(lens.max()) if n else 1)
    buf = np.zeros((max(n, 1), stride), np.uint8)
    for i, d in enumerate(datas):
        buf[i, :len(d)] = np.frombuffer(bytes(d), np.uint8)
    out = np.zeros((n, n_out), np.float32)
    pc = np.zeros((n, n_out), np.int16) if pcm else None
    rc = call(ptr(buf), stride, ptr(lens), n, ptr(out), n_out, n_out, ptr(pc) if pcm else None, n_out)
    return rc, ((out, pc) if pcm else out)


def modulate(mode: int, datas, baud, f0, f1=0.0, samp_rate=96000, n_out=None, pcm=False):
    """Batched transmit side on the GPU (amr_modulate_host): the reference
    modulator's float32 waveform of every payload in `datas` (modem.py:28-65,
    138-186, 270-295), cut / zero-padded to n_out samples (default: the
    longest natural length).  pcm=True also returns wav_from_array's int16."""
    require_gpu()
    if n_out is None:
        n_out = max((tx_samples(mode, len(d), baud, samp_rate) for d in datas), default=0)
    rc, res = _modulate_call(datas, n_out, pcm, lambda *a: lib().amr_modulate_host(
        mode, float(baud), float(f0), float(f1), float(samp_rate), *a))
    if rc != AMR_OK:
        _raise_tx(rc)
    return res


def psk_slice(kind: str, sym: np.ndarray) -> np.ndarray:
    """The slicer stage alone on the GPU (K4a): sym [B][S] complex128 -> the
    decided bits [B][bits] as uint8 (modem.py:214-241 QPSK, :100-105 BPSK;
    "d8psk": k_slice8's eight sectors, 3 bits per product; "star16":
    k_slice16's ring bit and tribit, 4 per product)."""
    require_gpu()
    sym = np.ascontiguousarray(np.atleast_2d(sym), np.complex128)
    B, S = sym.shape
    nbits = max(0, (S - 1) * psk_bits(kind))
    nw = max(1, (nbits + 31) // 32)
    words = np.zeros((B, nw), np.uint32)
    check(lib().amr_psk_slice_host(psk_kind(kind), ptr(sym), B, S, ptr(words)))
    bits = np.unpackbits(words.astype(">u4").view(np.uint8).reshape(B, -1), axis=1)
    return bits[:, :nbits]


def sync_pack(bits, n_words=None, out_stride=None, fill=0xA5, n_bits=None):
    """The sync search and byte pack alone on the GPU (k_sync_pack through
    amr_sync_pack_host): bits [B][n_bits] of 0/1 -> (out [B][out_stride] uint8,
    out_len [B], sync_idx [B]).  out is pre-filled with `fill` and returned
    whole, so a caller can look past out_len.  n_words (default ceil(n_bits/32),
    at least 1) and out_stride (default n_bits // 8) size the two buffers.
    With n_bits given, `bits` may be wider, up to n_words * 32 columns: the
    columns past n_bits are stale data the kernel must not read."""
    require_gpu()
    bits = np.ascontiguousarray(np.atleast_2d(bits), np.uint8)
    B = bits.shape[0]
    n_bits = bits.shape[1] if n_bits is None else int(n_bits)
    nw = max(1, (n_bits + 31) // 32) if n_words is None else int(n_words)
    stride = n_bits // 8 if out_stride is None else int(out_stride)
    if not n_bits <= bits.shape[1] <= max(nw * 32, n_bits):
        raise ValueError("sync_pack: bits holds n_bits to n_words * 32 columns")
    words = pack_words(bits, nw)
    out = np.full((B, max(stride, 0)), fill, np.uint8)
    ln = np.zeros(B, np.int64)
    sync = np.zeros(B, np.int64)
    check(lib().amr_set_device(default_device()))
    check(lib().amr_sync_pack_host(ptr(words), B, nw, n_bits, ptr(out), stride, ptr(ln), ptr(sync)))
    return out, ln, sync


def pack_words(bits: np.ndarray, n_words: int) -> np.ndarray:
    """bits [B][n] of 0/1 as [B][n_words] uint32, MSB first, zero past n (host
    only; psk_slice's unpacking the other way round).  A row too long for
    n_words is cut, so that the library sees, and refuses, the short n_words."""
    B, n = bits.shape
    full = np.zeros((B, n_words * 32), np.uint8)
    full[:, :min(n, n_words * 32)] = bits[:, :n_words * 32]
    return np.packbits(full, axis=1).reshape(B, n_words, 4).view(">u4").astype(np.uint32).reshape(B, n_words)


def frame_parse(raws, max_cands: int = 64):
    """Batched decoder.parse_fbp_stream_enhanced scan (decoder.py:142-208) on
    the GPU: for each bytes object, (n_candidates, records[:min(n, max_cands)])
    with the reference's per-candidate verdict (FRAME_*) and header fields."""
    require_gpu()
    n = len(raws)
    if n == 0:
        return []
    lens = np.array([len(r) for r in raws], np.int64)
    stride = max(1, int(lens.max()))
    buf = np.zeros((n, stride), np.uint8)
    for i, r in enumerate(raws):
        buf[i, :len(r)] = np.frombuffer(r, np.uint8)
    cnt = np.zeros(n, np.int32)
    recs = np.zeros((n, max_cands), FRAME_REC)
    check(lib().amr_frame_parse_host(ptr(buf), stride, ptr(lens), n, max_cands, ptr(cnt), recs.ctypes.data))
    return [(int(cnt[i]), recs[i, :min(int(cnt[i]), max_cands)]) for i in range(n)]


class PinnedArray:
    """A numpy array over page-locked host memory (amr_host_alloc): the buffer
    a capture loop fills and hands to the *_demod_host_async entries."""

    def __init__(self, shape, dtype):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = ctypes.c_void_p()
        check(lib().amr_host_alloc(ctypes.byref(self._p), max(1, self.nbytes)))
        buf = (ctypes.c_uint8 * max(1, self.nbytes)).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if self._p:
            self.array = None
            lib().amr_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AmrError(RuntimeError):
    """A libamr.so call failed (message from amr_last_error)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"libamr error {code}: {msg}")
        self.code = code


_lib = None
_lib_lock = threading.Lock()
P, I64, I32, D, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_float


def lib():
    """Load libamr.so (raises if it was never built -- there is no fallback)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise AmrError(AMR_E_NODEVICE, f"{LIB_PATH} not found: build it with "
                                           "`python audio-modem-radio_amd/build.py` (there is no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        sig = {
            "amr_abi_version": (I32, []),
            "amr_build_id": (ctypes.c_char_p, []),
            "amr_last_error": (ctypes.c_char_p, []),
            "amr_device_count": (I32, [P]),
            "amr_set_device": (I32, [I32]),
            "amr_malloc": (I32, [P, I64]),
            "amr_free": (I32, [P]),
            "amr_memcpy_h2d": (I32, [P, P, I64]),
            "amr_memcpy_d2h": (I32, [P, P, I64]),
            "amr_memcpy_d2d": (I32, [P, P, I64]),
            "amr_device_synchronize": (I32, []),
            "amr_psk_plan_create": (I32, [P, I32, I32, I64, I64, I64, P, P, P, I32, P, P, P, I32, P, I64]),
            "amr_psk_plan_destroy": (I32, [P]),
            "amr_psk_plan_out_capacity": (I64, [P]),
            "amr_psk_plan_scratch_bytes": (I64, [P]),
            "amr_psk_plan_bytes_estimate": (I64, [I32, I64, I64, I64, I32, I32, I64]),
            "amr_fsk_plan_bytes_estimate": (I64, [I64, I64, I32, I64]),
            "amr_psk_plan_synchronize": (I32, [P]),
            "amr_psk_plan_enable_timing": (I32, [P, I32]),
            "amr_psk_plan_set_inflight": (I32, [P, I32]),
            "amr_psk_plan_timings": (I32, [P, P, I32]),
            "amr_psk_plan_exact_streams": (I32, [P, P]),
            "amr_psk_demod_host": (I32, [P, P, I32, I64, I64, P, I64, P, P]),
            "amr_psk_demod_device": (I32, [P, P, I32, I64, I64, P, I64, P, P]),
            "amr_psk_demod_host_edges": (I32, [P, P, I32, I64, I64, P, P, I64, P, P]),
            "amr_psk_demod_device_edges": (I32, [P, P, I32, I64, I64, P, P, I64, P, P]),
            "amr_fsk_demod_host_edges": (I32, [P, P, I32, I64, I64, P, P, I64, P, P]),
            "amr_fsk_demod_device_edges": (I32, [P, P, I32, I64, I64, P, P, I64, P, P]),
            "amr_psk_split_bounds_host": (I32, [P, P, I32, I64, I64, P, P, P]),
            "amr_psk_plan_set_split_strict": (I32, [P, I32]),
            "amr_psk_plan_split_strict": (I32, [P]),
            "amr_psk_plan_last_strict": (I32, [P]),
            "amr_psk_split_strict_design": (I32, [P, P, P, I32, P, P, P, I32, I64, I64, I64, P, P]),
            "amr_psk_demod_fec_device": (I32, [P, P, I32, I64, I64, P, I64, P, P, P, I64, P, P]),
            "amr_psk_slice_host": (I32, [I32, P, I64, I64, P]),
            "amr_sync_pack_host": (I32, [P, I64, I64, I64, P, I64, P, P]),
            "amr_psk_plan_last_layout": (I32, [P]),
            "amr_psk_plan_set_layout": (I32, [P, I32]),
            "amr_psk_plan_split_info": (I32, [P, P, P, P, P, P]),
            "amr_psk_split_design": (I32, [P, P, I32, P, P, I32, I64, I64, P, P, P]),
            "amr_psk_split_symbols_host": (I32, [P, P, I32, I64, I64, I64, P]),
            "amr_split_state_tables": (I32, [P, P, P, I32, I64, P, P]),
            "amr_psk_plan_split_conv": (I32, [P]),
            "amr_psk_f32_margin": (D, [P, P, I32]),
            "amr_psk_plan_last_f32f": (I32, [P]),
            "amr_psk_plan_last_lowpass": (I32, [P]),
            "amr_psk_demod_host_async": (I32, [P, P, I32, I64, I64, P, I64, P, P]),
            "amr_fsk_demod_host_async": (I32, [P, P, I32, I64, I64, P, I64, P, P]),
            "amr_host_register": (I32, [P, I64]),
            "amr_host_alloc": (I32, [P, I64]),
            "amr_host_free": (I32, [P]),
            "amr_host_unregister": (I32, [P]),
            "amr_synth_tile_noise": (I32, [P, I64, I64, P, I64, I64, F, ctypes.c_uint64]),
            "amr_fsk_plan_create": (I32, [P, I32, I64, I64, P, P, P, P, P, P, I32, I64]),
            "amr_fsk_plan_destroy": (I32, [P]),
            "amr_fsk_plan_out_capacity": (I64, [P]),
            "amr_fsk_plan_scratch_bytes": (I64, [P]),
            "amr_fsk_plan_resident_bytes": (I64, [P]),
            "amr_fsk_plan_fft_length": (I64, [P]),
            "amr_fsk_plan_live_columns": (I32, [P]),
            "amr_fsk_plan_synchronize": (I32, [P]),
            "amr_fsk_plan_enable_timing": (I32, [P, I32]),
            "amr_fsk_plan_timings": (I32, [P, P, I32]),
            "amr_fsk_demod_host": (I32, [P, P, I32, I64, I64, P, I64, P, P]),
            "amr_fsk_demod_device": (I32, [P, P, I32, I64, I64, P, I64, P, P]),
            "amr_fsk_envelopes_host": (I32, [P, P, I32, I64, I64, P, P]),
            "amr_fft_c2c_host": (I32, [P, P, I64, I64, I32, I32]),
            "amr_hilbert_host": (I32, [P, P, I64, I64, I32]),
            "amr_fec_decode_host": (I32, [P, I64, P, I64, P, I64, P, P]),
            "amr_frame_parse_host": (I32, [P, I64, P, I64, I64, P, P]),
            "amr_frame_parse_device": (I32, [P, P, I64, P, I64, I64, P, P]),
            "amr_comm_unique_id": (I32, [P]),
            "amr_comm_create": (I32, [P, P, I32, I32, I32]),
            "amr_comm_destroy": (I32, [P]),
            "amr_allgather": (I32, [P, P, P, I64, P]),
            "amr_fsk_allgather": (I32, [P, P, P, I64, P]),
            "amr_comm_synchronize": (I32, [P]),
            "amr_comm_allgather_host": (I32, [P, P, P, I64]),
            "amr_comm_allreduce_max": (I32, [P, P, I64]),
            "amr_comm_world": (I32, [P, P, P]),
            "amr_tx_samples": (I64, [I32, I64, D, D]),
            "amr_resample_host": (I32, [P, I64, I64, I64, P, I32]),
            "amr_hilbert_env_exact_host": (I32, [P, I64, I64, P, I32]),
            "amr_fsk_plan_exact_streams": (I32, [P, P]),
            "amr_fsk_plan_set_exact_mode": (I32, [P, I32]),
            "amr_fsk_plan_set_layout": (I32, [P, I32]),
            "amr_fsk_plan_split_info": (I32, [P, P, P, P, P, P]),
            "amr_fsk_split_design": (I32, [I64, P, P, P, P, I32, P, P, P]),
            "amr_fsk_fft_margin": (I32, [I64, P, P, P, P, P, P, I32, P]),
            "amr_fsk_plan_margin": (I32, [P, P, P]),
            "amr_fsk_plan_set_split_strict": (I32, [P, I32]),
            "amr_fsk_plan_split_strict": (I32, [P]),
            "amr_fsk_plan_last_strict": (I32, [P]),
            "amr_fsk_split_strict_design": (I32, [P, P, P, I32, I64, P, P]),
            "amr_fsk_split_bounds_host": (I32, [P, P, I32, I64, I64, P, P, P]),
            "amr_fsk_split_bandpass_host": (I32, [P, P, I32, I64, I64, I64, P]),
            "amr_fsk_plan_split_conv": (I32, [P]),
            "amr_tx_work_bytes": (I64, [I32, D, D, I64, I64]),
            "amr_modulate_host": (I32, [I32, D, D, D, D, P, I64, P, I64, P, I64, I64, P, I64]),
            "amr_modulate_device": (I32, [P, I32, D, D, D, D, P, I64, P, I64, P, I64, I64, P, I64, P, I64]),
            "amr_hell_pixels": (I64, [I64, D, D]),
            "amr_hell_work_bytes": (I64, [D, D]),
            "amr_hell_demod_host": (I32, [P, I32, I64, I64, I64, D, D, P, I64, P, P]),
            "amr_hell_demod_device": (I32, [P, P, I32, I64, I64, I64, D, D, P, I64, P, P, P, I64]),
            "amr_hell_glyph_rows": (I32, [P, P]),
            "amr_conv_encoded_len": (I64, [I64]),
            "amr_conv_encode_host": (I32, [P, I64, P, I64, P, I64, P]),
            "amr_viterbi_work_bytes": (I64, [I64, I64]),
            "amr_viterbi_decode_device": (I32, [P, P, I64, P, I64, P, I64, P, P, P, I64]),
            "amr_viterbi_decode_host": (I32, [P, I64, P, I64, P, I64, P, P]),
            "amr_psk_demod_soft_host": (I32, [P, P, I32, I64, I64, P, I64, P, P, P, P, I64]),
            "amr_psk_demod_soft_device": (I32, [P, P, I32, I64, I64, P, I64, P, P, P, P, I64]),
            "amr_psk_soft_host": (I32, [I32, P, I64, I64, P]),
            "amr_viterbi_soft_work_bytes": (I64, [I64, I64]),
            "amr_viterbi_decode_soft_device": (I32, [P, P, I64, I64, P, I64, P, I64, P, P, P, I64]),
            "amr_viterbi_decode_soft_host": (I32, [P, I64, I64, P, I64, P, I64, P, P]),
            "amr_rs_encoded_len": (I64, [I64, I32]),
            "amr_rs_decoded_len": (I64, [I64, I32]),
            "amr_rs_encode_host": (I32, [P, I64, P, I64, I32, I32, P, I64, P]),
            "amr_rs_encode_device": (I32, [P, P, I64, P, I64, I32, I32, P, I64, P]),
            "amr_rs_decode_host": (I32, [P, I64, P, P, I64, I32, I32, P, I64, P, P, P]),
            "amr_rs_decode_device": (I32, [P, P, I64, P, P, I64, I32, I32, P, I64, P, P, P]),
            "amr_ofdm_plan_create": (I32, [P, I32, I64, I64, I32, P, P, I64]),
            "amr_ofdm_plan_destroy": (I32, [P]),
            "amr_ofdm_plan_synchronize": (I32, [P]),
            "amr_ofdm_plan_enable_timing": (I32, [P, I32]),
            "amr_ofdm_plan_timings": (I32, [P, P, I32]),
            "amr_ofdm_plan_out_capacity": (I64, [P]),
            "amr_ofdm_plan_scratch_bytes": (I64, [P]),
            "amr_ofdm_plan_bytes_estimate": (I64, [I64, I64, I32, I64]),
            "amr_ofdm_demod_host": (I32, [P, P, I32, I64, I64, P, I64, P, P]),
            "amr_ofdm_demod_device": (I32, [P, P, I32, I64, I64, P, I64, P, P]),
            "amr_ofdm_demod_soft_host": (I32, [P, P, I32, I64, I64, P, I64, P, P, P, I64]),
            "amr_ofdm_demod_soft_device": (I32, [P, P, I32, I64, I64, P, I64, P, P, P, I64]),
            "amr_ofdm_symbols_host": (I32, [P, P, I32, I64, I64, P]),
            "amr_ofdm_slice_host": (I32, [P, I64, I64, I32, P]),
            "amr_ofdm_soft_host": (I32, [P, I64, I64, I32, P]),
            "amr_ofdm_modulate_host": (I32, [D, D, D, I32, P, I64, P, I64, P, I64, I64, P, I64]),
            "amr_ofdm_acquire_bytes_estimate": (I64, [I64, I64, I32, I64]),
            "amr_ofdm_acquire_host": (I32, [P, P, I32, I64, I64, P, P, P]),
            "amr_ofdm_acquire_device": (I32, [P, P, I32, I64, I64, P, P, P]),
            "amr_ofdm_symbols_at_host": (I32, [P, P, I32, I64, I64, P, P]),
            "amr_ofdm_demod_acq_host": (I32, [P, P, I32, I64, I64, P, I64, P, P, P, I64, P]),
            "amr_ofdm_demod_acq_device": (I32, [P, P, I32, I64, I64, P, I64, P, P, P, I64, P]),
            "amr_dsss_plan_create": (I32, [P, I32, I64, I64, I32, I64, P, P, P, I64]),
            "amr_dsss_plan_destroy": (I32, [P]),
            "amr_dsss_plan_synchronize": (I32, [P]),
            "amr_dsss_plan_enable_timing": (I32, [P, I32]),
            "amr_dsss_plan_timings": (I32, [P, P, I32]),
            "amr_dsss_plan_out_capacity": (I64, [P]),
            "amr_dsss_plan_scratch_bytes": (I64, [P]),
            "amr_dsss_plan_bytes_estimate": (I64, [I64, I64, I32, I64]),
            "amr_dsss_acquire_bytes_estimate": (I64, [I64, I64, I32, I64]),
            "amr_dsss_demod_host": (I32, [P, P, I32, I64, I64, P, I64, P, P, P, I64, P, I32]),
            "amr_dsss_demod_device": (I32, [P, P, I32, I64, I64, P, I64, P, P, P, I64, P, I32]),
            "amr_dsss_acquire_host": (I32, [P, P, I32, I64, I64, P, P]),
            "amr_dsss_acquire_device": (I32, [P, P, I32, I64, I64, P, P]),
            "amr_dsss_symbols_at_host": (I32, [P, P, I32, I64, I64, P, P]),
            "amr_dsss_slice_host": (I32, [P, I64, I64, P]),
            "amr_dsss_soft_host": (I32, [P, I64, I64, P]),
            "amr_dsss_modulate_host": (I32, [I64, I32, I64, P, P, P, I64, P, I64, P, I64, I64, P, I64]),
            "amr_msk_plan_create": (I32, [P, I32, I64, I64, I64, P, P, P, P, I64]),
            "amr_msk_plan_destroy": (I32, [P]),
            "amr_msk_plan_synchronize": (I32, [P]),
            "amr_msk_plan_enable_timing": (I32, [P, I32]),
            "amr_msk_plan_timings": (I32, [P, P, I32]),
            "amr_msk_plan_out_capacity": (I64, [P]),
            "amr_msk_plan_scratch_bytes": (I64, [P]),
            "amr_msk_plan_bytes_estimate": (I64, [I64, I64, I64]),
            "amr_msk_acquire_bytes_estimate": (I64, [I64, I64, I64]),
            "amr_msk_demod_host": (I32, [P, P, I32, I64, I64, P, I64, P, P, P, I64, P, I32]),
            "amr_msk_demod_device": (I32, [P, P, I32, I64, I64, P, I64, P, P, P, I64, P, I32]),
            "amr_msk_acquire_host": (I32, [P, P, I32, I64, I64, P, P]),
            "amr_msk_acquire_device": (I32, [P, P, I32, I64, I64, P, P]),
            "amr_msk_symbols_at_host": (I32, [P, P, I32, I64, I64, P, P]),
            "amr_msk_offset_host": (I32, [I64, P, P, I64, P, P]),
            "amr_msk_slice_host": (I32, [P, I64, I64, I64, P]),
            "amr_msk_soft_host": (I32, [P, I64, I64, I64, P]),
            "amr_msk_modulate_host": (I32, [I64, I64, P, P, I64, P, I64, P, I64, I64, P, I64]),
            "amr_tone8_chunk": (I64, [I64]),
            "amr_tone8_plan_create": (I32, [P, I32, I64, I64, I64, I64, P, I64]),
            "amr_tone8_plan_destroy": (I32, [P]),
            "amr_tone8_plan_synchronize": (I32, [P]),
            "amr_tone8_plan_enable_timing": (I32, [P, I32]),
            "amr_tone8_plan_timings": (I32, [P, P, I32]),
            "amr_tone8_plan_out_capacity": (I64, [P]),
            "amr_tone8_plan_scratch_bytes": (I64, [P]),
            "amr_tone8_plan_bytes_estimate": (I64, [I64, I64, I64, I64]),
            "amr_tone8_acquire_bytes_estimate": (I64, [I64, I64, I64, I64]),
            "amr_tone8_demod_host": (I32, [P, P, I32, I64, I64, P, I64, P, P, P, I64, P, P, I32]),
            "amr_tone8_demod_device": (I32, [P, P, I32, I64, I64, P, I64, P, P, P, I64, P, P, I32]),
            "amr_tone8_acquire_host": (I32, [P, P, I32, I64, I64, P, P, P]),
            "amr_tone8_acquire_device": (I32, [P, P, I32, I64, I64, P, P, P]),
            "amr_tone8_symbols_at_host": (I32, [P, P, I32, I64, I64, P, P, P]),
            "amr_tone8_peak_host": (I32, [I64, I64, P, I64, I64, P, P, P]),
            "amr_tone8_slice_host": (I32, [P, I64, I64, P]),
            "amr_tone8_soft_host": (I32, [P, I64, I64, P]),
            "amr_tone8_modulate_host": (I32, [I64, I64, P, P, I64, P, I64, P, I64, I64, P, I64]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
        return L


def check(rc: int):
    if rc != AMR_OK:
        raise AmrError(rc, lib().amr_last_error().decode("utf-8", "replace"))
    return rc


def ptr(a) -> ctypes.c_void_p:
    return ctypes.c_void_p(a.ctypes.data)


def is_kernel_dtype(dt) -> bool:
    """float32 / float64: the dtypes the kernels read and extend themselves."""
    return np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.float64))


def raw_input(x: np.ndarray, pad: int):
    """A raw capture [B][n] of any other real dtype -- integers of every width
    (int16 as its values, not PCM), bool, float16, longdouble -- as the
    reference's filtfilt sees it (modem.py:77, 198, 308; scipy
    _arraytools.odd_ext): (xk, edges).  xk: the samples as float32 (exact for
    integers of <= 16 bits, bool, float16) or float64 (numpy's cast, which is
    lfilter's own); edges [B][2 pad] float64: the odd extension 2*x[0] - x[k]
    computed by numpy IN x's dtype -- integer wraparound, bool -> int64,
    float16 rounding -- the left pad then the right (include/amr.h
    amr_psk_demod_host_edges).  n > pad (the plan's design checked it)."""
    x = np.ascontiguousarray(x)
    if not x.dtype.isnative:
        x = np.ascontiguousarray(x.astype(x.dtype.newbyteorder("=")))
    pad = int(pad)
    with np.errstate(all="ignore"):                      # numpy warns where scipy would, e.g. float16 overflow
        left = 2 * x[:, :1] - x[:, pad:0:-1]             # ext index j < pad: 2 x[0] - x[pad - j]
        right = 2 * x[:, -1:] - x[:, -2:-(pad + 2):-1]    # ext index pad + n + r: 2 x[n-1] - x[n-2-r]
        edges = np.ascontiguousarray(np.concatenate([left, right], axis=1), np.float64)
    narrow = x.dtype.kind == "b" or (x.dtype.kind in "iu" and x.dtype.itemsize <= 2) or x.dtype == np.float16
    return np.ascontiguousarray(x, np.float32 if narrow else np.float64), edges


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = lib().amr_device_count(ctypes.byref(n))
    return n.value if rc == AMR_OK else 0


def default_device() -> int:
    for k in ("AMR_DEVICE", "LOCAL_RANK"):
        if k in os.environ:
            return int(os.environ[k])
    return 0


def require_gpu():
    if device_count() < 1:
        raise AmrError(AMR_E_NODEVICE, "no GPU visible to libamr.so: the demodulator runs only on the "
                                       "MI355X (there is no CPU fallback)")


# ---------------------------------------------------------------------------
# filter design (host, scipy) -- exactly the reference's calls
def design_psk(kind: str, n: int, baud, carrier=3000.0, samp_rate=96000):
    """Return (sps, first, bp(b,a,zi), lp(b,a,zi), lo4) or raise scipy's ValueError.

    Order of the reference's failure points is kept: band-pass design,
    band-pass filtfilt padlen check, low-pass design (modem.py:76-88 / 197-204)."""
    from scipy import signal
    psk_kind(kind)                                       # KeyError names an unknown kind
    sps = int(samp_rate / baud)
    nyq = samp_rate / 2
    if kind in ("qpsk", "d8psk", "star16"):
        low = (carrier - baud * 1.5) / nyq
        high = (carrier + baud * 1.5) / nyq
        first = sps // 2
    else:
        low = (carrier - baud) / nyq
        high = (carrier + baud) / nyq
        first = sps
    b, a = signal.butter(4, [max(0.01, low), min(0.99, high)], btype="band")
    ntaps = max(len(a), len(b))
    if n <= 3 * ntaps:
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % (3 * ntaps))
    bl, al = signal.butter(4, baud / nyq, btype="low")
    bp = tuple(np.ascontiguousarray(v, np.float64) for v in (b, a, signal.lfilter_zi(b, a)))
    lp = tuple(np.ascontiguousarray(v, np.float64) for v in (bl, al, signal.lfilter_zi(bl, al)))
    return sps, first, bp, lp, lo_table(n, carrier, samp_rate)


def split_design(kind: str, n: int, baud, carrier=3000.0, samp_rate=96000):
    """The time-split design (host arithmetic in libamr.so, no device): dict of
    warmup_bp, warmup_lp, kappa, or None when the filters do not allow it."""
    sps, first, bp, lp, _ = design_psk(kind, n, baud, carrier, samp_rate)
    S = max(0, (n - first + sps - 1) // sps)
    w1, w2 = ctypes.c_int64(), ctypes.c_int64()
    k = ctypes.c_double()
    rc = lib().amr_psk_split_design(ptr(bp[0]), ptr(bp[1]), len(bp[0]), ptr(lp[0]), ptr(lp[1]), len(lp[0]), n, S,
                                    ctypes.byref(w1), ctypes.byref(w2), ctypes.byref(k))
    return None if rc != 0 else {"warmup_bp": w1.value, "warmup_lp": w2.value, "kappa": k.value}


def state_tables(b, a, zi, w: int):
    """amr_split_state_tables for one DF-II-T filter: (K [w][nt-1], Z0 [w+1][nt-1])."""
    b, a, zi = (np.ascontiguousarray(v, np.float64) for v in (b, a, zi))
    K, Z0 = np.zeros((w, len(b) - 1)), np.zeros((w + 1, len(b) - 1))
    check(lib().amr_split_state_tables(ptr(b), ptr(a), ptr(zi), len(b), int(w), ptr(K), ptr(Z0)))
    return K, Z0


def split_state_tables(kind: str, n: int, baud, carrier=3000.0, samp_rate=96000):
    """The time-split band-pass's convolution tables (K [w1][8], Z0 [w1 + 1][8];
    libamr.so host arithmetic, amr_split_state_tables), or None without a design."""
    d = split_design(kind, n, baud, carrier, samp_rate)
    if d is None:
        return None
    _, _, bp, _, _ = design_psk(kind, n, baud, carrier, samp_rate)
    w = d["warmup_bp"]
    ns = len(bp[0]) - 1
    K, Z0 = np.zeros((w, ns)), np.zeros((w + 1, ns))
    check(lib().amr_split_state_tables(ptr(bp[0]), ptr(bp[1]), ptr(bp[2]), len(bp[0]), w, ptr(K), ptr(Z0)))
    return K, Z0


STRICT_CONSTS = ["g1x", "gmax", "hz", "tk", "zi_sum", "zb", "kx", "ky", "u2", "gam", "c3", "w1", "w2", "n_sym", "nw",
                 "nk", "nh", "ng", "nz", "k12_off", "w_tail", "k12_tail", "hs_tail", "tz_tail", "lp_tail", "lp_rad",
                 "ok", "kappa"]


def split_strict_design(kind: str, n: int, baud, carrier=3000.0, samp_rate=96000):
    """The strict bound's design (libamr.so host arithmetic, amr_psk_split_strict_design):
    dict of the constants and the tables kabs, z0abs, lpc, W, K12, HS, GS, TZ; None
    when the plan has no strict bound."""
    sps, first, bp, lp, _ = design_psk(kind, n, baud, carrier, samp_rate)
    c = np.zeros(32)
    args = [ptr(bp[0]), ptr(bp[1]), ptr(bp[2]), len(bp[0]), ptr(lp[0]), ptr(lp[1]), ptr(lp[2]), len(lp[0]), n, first,
            sps, ptr(c)]
    if lib().amr_psk_split_strict_design(*args, None) != 0:
        return None
    d = dict(zip(STRICT_CONSTS, c[:len(STRICT_CONSTS)].tolist()))
    sizes = [("kabs", int(d["w1"])), ("z0abs", int(d["w1"]) + 1), ("lpc", int(d["n_sym"])), ("W", int(d["nw"])),
             ("K12", int(d["nk"])), ("HS", int(d["nh"])), ("GS", int(d["ng"])), ("TZ", int(d["nz"]))]
    tabs = np.zeros(sum(k for _, k in sizes))
    check(lib().amr_psk_split_strict_design(*args, ptr(tabs)))
    o = 0
    for name, k in sizes:
        d[name] = tabs[o:o + k]
        o += k
    return d


def f32_margin(kind: str, n: int, baud, carrier=3000.0, samp_rate=96000) -> float:
    """The float32 hand-off's symbol error bound per unit max |f| (libamr.so, host arithmetic)."""
    _, _, _, lp, _ = design_psk(kind, n, baud, carrier, samp_rate)
    return float(lib().amr_psk_f32_margin(ptr(lp[0]), ptr(lp[1]), len(lp[0])))


def lo_table(n: int, carrier, samp_rate) -> np.ndarray:
    """[n][4]: lo_re, lo_im, -(0*lo_im), 0*lo_re with lo = exp(-1j*2*pi*fc*t) (modem.py:200-201).

    The last two columns are the addends numpy's complex multiply
    (filtered + 0j) * lo evaluates: re = fma(f, lo_re, -(0*lo_im)),
    im = fma(f, lo_im, 0*lo_re)."""
    t = np.arange(n) / samp_rate
    lo = np.exp(-1j * 2 * np.pi * carrier * t)
    out = np.empty((n, 4))
    out[:, 0] = lo.real
    out[:, 1] = lo.imag
    out[:, 2] = -(0.0 * lo.imag)
    out[:, 3] = 0.0 * lo.real
    return out


class PskPlan:
    """A device plan: coefficients + LO in HBM + scratch for max_streams streams."""

    def __init__(self, kind: str, n: int, baud, carrier=3000.0, samp_rate=96000, max_streams=64,
                 device=None):
        self.kind, self.n, self.baud, self.carrier, self.samp_rate = kind, n, baud, carrier, samp_rate
        self.sps, self.first, self.bp, self.lp, lo4 = design_psk(kind, n, baud, carrier, samp_rate)
        require_gpu()
        self.device = default_device() if device is None else device
        self.max_streams = int(max_streams)
        h = ctypes.c_void_p()
        b, a, zi = self.bp
        bl, al, zil = self.lp
        check(lib().amr_psk_plan_create(ctypes.byref(h), self.device, psk_kind(kind),
                                        n, self.sps, self.first, ptr(b), ptr(a), ptr(zi), len(b),
                                        ptr(bl), ptr(al), ptr(zil), len(bl), ptr(lo4), self.max_streams))
        self.handle = h
        self.out_cap = int(lib().amr_psk_plan_out_capacity(h))
        self.lock = threading.Lock()

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and _lib is not None:
            try:
                _lib.amr_psk_plan_destroy(h)
            except Exception:
                pass
            self.handle = None

    def demod_host(self, x: np.ndarray):
        """x [B][N] float32/float64/int16 (int16 = PCM read as int16/32768). Returns (list[bytes], sync)."""
        x = np.ascontiguousarray(x)
        dt = DTYPES
        B = x.shape[0]
        outs, syncs = [], np.empty(B, np.int64)
        cap = max(self.out_cap, 1)
        for s0 in range(0, B, self.max_streams):
            xb = x[s0:s0 + self.max_streams]
            nb = xb.shape[0]
            out = np.empty((nb, cap), np.uint8)
            ln = np.empty(nb, np.int64)
            sy = np.empty(nb, np.int64)
            with self.lock:
                check(lib().amr_psk_demod_host(self.handle, ptr(xb), dt[xb.dtype], nb, xb.shape[1], ptr(out), cap,
                                               ptr(ln), ptr(sy)))
            outs += [out[i, :ln[i]].tobytes() for i in range(nb)]
            syncs[s0:s0 + nb] = sy
        return outs, syncs

    def demod_host_raw(self, x: np.ndarray):
        """x [B][N] of a dtype the kernels do not store (raw_input): the
        reference's semantics for that array.  Returns (list[bytes], sync)."""
        xk, edges = raw_input(np.atleast_2d(x), 3 * len(self.bp[0]))
        B = xk.shape[0]
        outs, syncs = [], np.empty(B, np.int64)
        cap = max(self.out_cap, 1)
        for s0 in range(0, B, self.max_streams):
            xb, eb = xk[s0:s0 + self.max_streams], edges[s0:s0 + self.max_streams]
            nb = xb.shape[0]
            out = np.empty((nb, cap), np.uint8)
            ln = np.empty(nb, np.int64)
            sy = np.empty(nb, np.int64)
            with self.lock:
                check(lib().amr_psk_demod_host_edges(self.handle, ptr(xb), DTYPES[xb.dtype], nb, xb.shape[1],
                                                     ptr(eb), ptr(out), cap, ptr(ln), ptr(sy)))
            outs += [out[i, :ln[i]].tobytes() for i in range(nb)]
            syncs[s0:s0 + nb] = sy
        return outs, syncs

    def _demod_soft(self, xk: np.ndarray, edges):
        B = xk.shape[0]
        outs, softs, syncs = [], [], np.empty(B, np.int64)
        cap = max(self.out_cap, 1)
        for s0 in range(0, B, self.max_streams):
            xb = xk[s0:s0 + self.max_streams]
            eb = None if edges is None else edges[s0:s0 + self.max_streams]
            nb = xb.shape[0]
            out = np.empty((nb, cap), np.uint8)
            soft = np.empty((nb, 8 * cap), np.int8)
            ln = np.empty(nb, np.int64)
            sy = np.empty(nb, np.int64)
            with self.lock:
                check(lib().amr_psk_demod_soft_host(self.handle, ptr(xb), DTYPES[xb.dtype], nb, xb.shape[1], ptr(out),
                                                    cap, ptr(ln), ptr(sy), None if eb is None else ptr(eb),
                                                    ptr(soft), 8 * cap))
            outs += [out[i, :ln[i]].tobytes() for i in range(nb)]
            softs += [soft[i, :8 * ln[i]].copy() for i in range(nb)]
            syncs[s0:s0 + nb] = sy
        return outs, syncs, softs

    def demod_soft_host(self, x: np.ndarray):
        """demod_host with the soft values (amr_psk_demod_soft_host):
        (list[bytes], sync, list[int8 array]); soft[i][j] belongs to bit j of
        outs[i], so np.packbits(soft[i] > 0) is outs[i] again."""
        return self._demod_soft(np.ascontiguousarray(x), None)

    def demod_soft_host_raw(self, x: np.ndarray):
        """demod_host_raw with the soft values."""
        xk, edges = raw_input(np.atleast_2d(x), 3 * len(self.bp[0]))
        return self._demod_soft(xk, edges)

    def scratch_bytes(self) -> int:
        """Device bytes this plan holds (scratch + host-API staging)."""
        return int(lib().amr_psk_plan_scratch_bytes(self.handle)) if self.handle else 0

    def enable_timing(self, on=True):
        check(lib().amr_psk_plan_enable_timing(self.handle, 1 if on else 0))

    def set_inflight(self, batches: int):
        """Hint: `batches` batches are kept in flight at once, each on its own plan."""
        check(lib().amr_psk_plan_set_inflight(self.handle, int(batches)))

    def timings(self) -> dict:
        ms = (ctypes.c_float * len(T_NAMES))()
        check(lib().amr_psk_plan_timings(self.handle, ms, len(T_NAMES)))
        return {k: float(v) for k, v in zip(T_NAMES, ms) if v >= 0}

    LAYOUTS = {"row": 0, "lane": 1, "split": 2}

    def last_layout(self) -> str:
        """'row' (state-per-lane kernels), 'lane' (one stream per lane) or 'split'
        (time-split passes, margin-checked, serial fallback) for the last call."""
        return {v: k for k, v in self.LAYOUTS.items()}.get(int(lib().amr_psk_plan_last_layout(self.handle)), "?")

    def set_layout(self, layout):
        """Force 'row' / 'lane' / 'split' for this plan's calls; None: by streams in flight."""
        check(lib().amr_psk_plan_set_layout(self.handle, -1 if layout is None else self.LAYOUTS[layout]))

    def split_symbols(self, x: np.ndarray, chunk: int = 0) -> np.ndarray:
        """Diagnostic: the time-split passes' symbol samples [B][S] complex (not bit-exact)."""
        x = np.ascontiguousarray(np.atleast_2d(x))
        B = x.shape[0]
        S = max(0, (self.n - self.first + self.sps - 1) // self.sps)
        sym = np.zeros((B, S, 2))
        with self.lock:
            check(lib().amr_psk_split_symbols_host(self.handle, ptr(x), DTYPES[x.dtype], B, x.shape[1], int(chunk),
                                                    ptr(sym)))
        return sym[..., 0] + 1j * sym[..., 1]

    def set_split_strict(self, on):
        """The time-split layout's strict bound for this plan: True / False, None = the
        process default (AMR_PSK_SPLIT_STRICT=1)."""
        check(lib().amr_psk_plan_set_split_strict(self.handle, -1 if on is None else (1 if on else 0)))

    def split_strict(self) -> bool:
        return int(lib().amr_psk_plan_split_strict(self.handle)) == 1

    def last_strict(self) -> bool:
        return int(lib().amr_psk_plan_last_strict(self.handle)) == 1

    def split_bounds(self, x: np.ndarray):
        """Diagnostic: the strict passes' symbols [B][S] complex, the bound e [B][S] on each
        component's |split - reference|, and per stream (E1, F, X, P3) (P3 < 0: caps failed)."""
        x = np.ascontiguousarray(np.atleast_2d(x))
        B = x.shape[0]
        S = max(0, (self.n - self.first + self.sps - 1) // self.sps)
        sym = np.zeros((B, S, 2))
        eb = np.zeros((B, S))
        sc = np.zeros((B, 4))
        with self.lock:
            check(lib().amr_psk_split_bounds_host(self.handle, ptr(x), DTYPES[x.dtype], B, x.shape[1], ptr(sym),
                                                  ptr(eb), ptr(sc)))
        return sym[..., 0] + 1j * sym[..., 1], eb, sc

    def last_f32f(self) -> bool:
        """The last call handed the band-pass output to the low-pass in float32."""
        return int(lib().amr_psk_plan_last_f32f(self.handle)) == 1

    LOWPASS = {0: "lane", 1: "lane_fused", 2: "lane_half"}           # AMR_LP_* (include/amr.h)

    def last_lowpass(self) -> str:
        """The lane layout's low-pass kernel of the last call ("none": it ran no lane low-pass)."""
        return self.LOWPASS.get(int(lib().amr_psk_plan_last_lowpass(self.handle)), "none")

    def split_conv(self) -> bool:
        """The time-split layout starts its band-pass chunks from convolution
        states (KS0) rather than warm-ups (AMR_PSK_SPLIT_CONV=0)."""
        return int(lib().amr_psk_plan_split_conv(self.handle)) == 1

    def split_info(self) -> dict:
        """The time-split layout: streams the last call flagged for the serial path
        (-1: that call ran another layout), warm-ups, chunk length, error bound kappa."""
        fl, w1, w2, L = (ctypes.c_int64() for _ in range(4))
        k = ctypes.c_double()
        check(lib().amr_psk_plan_split_info(self.handle, ctypes.byref(fl), ctypes.byref(w1), ctypes.byref(w2),
                                            ctypes.byref(L), ctypes.byref(k)))
        return {"flagged": fl.value, "warmup_bp": w1.value, "warmup_lp": w2.value, "chunk": L.value,
                "kappa": k.value}

    def exact_streams(self) -> int:
        c = ctypes.c_int64(0)
        check(lib().amr_psk_plan_exact_streams(self.handle, ctypes.byref(c)))
        return c.value


class PlanCache:
    """LRU of device plans bounded by the HBM they hold.

    The reference keeps no state between calls; a long-running receiver
    decoding captures of ever-different lengths (the live-capture path,
    filebeep_advanced_v2.py:324) must not accumulate one plan per length.
    Plans are kept while their summed device bytes (scratch_bytes(), incl.
    host-API staging) stay within `budget` and there are at most
    `max_entries` of them; the least recently used are dropped first (their
    HBM is released when the last caller holding one lets go of it)."""

    def __init__(self, budget_bytes: int, max_entries: int = 32):
        import collections
        self.budget = int(budget_bytes)
        self.max_entries = int(max_entries)
        self._d = collections.OrderedDict()
        self.lock = threading.Lock()

    def get(self, key, need: int, make, estimate=None):
        """The cached plan for key if it holds >= need streams, else make(need);
        before making it, plans are evicted until estimate(need) (the new
        plan's device bytes) fits beside the rest within the budget."""
        with self.lock:
            pl = self._d.get(key)
            if pl is not None and pl.max_streams >= need:
                self._d.move_to_end(key)
                return pl
            if pl is not None:
                del self._d[key]                    # too small: its scratch goes before the new one's
                pl = None
            self._evict(reserve=int(estimate(need)) if estimate else 0)
            pl = make(need)
            self._d[key] = pl
            self._evict(reserve=0, keep=key)
            return pl

    def reserve(self, key, nbytes: int):
        """Room for `nbytes` more that the plan under `key` is about to allocate: other plans are evicted
        until they fit beside the rest within the budget."""
        with self.lock:
            self._evict(reserve=int(nbytes), keep=key)

    def total_bytes(self) -> int:
        with self.lock:
            return self._total_unlocked()

    def _total_unlocked(self) -> int:
        return sum(p.scratch_bytes() for p in self._d.values())

    def __len__(self):
        return len(self._d)

    def clear(self):
        with self.lock:
            self._d.clear()

    def _evict(self, reserve: int, keep=None):
        total = sum(p.scratch_bytes() for p in self._d.values())
        while self._d and (total + reserve > self.budget or len(self._d) > self.max_entries):
            k = next(iter(self._d))
            if k == keep:
                if len(self._d) == 1:
                    break
                self._d.move_to_end(k)
                k = next(iter(self._d))
            total -= self._d.pop(k).scratch_bytes()


def _cache_budget() -> int:
    return int(float(os.environ.get("AMR_PLAN_CACHE_BYTES", 64e9)))


def stream_bucket(batch: int, cap: int) -> int:
    """Plan size for a batch: the next power of two (a single-stream call gets
    a one-stream plan), capped at `cap` streams per launch."""
    b = max(1, min(int(batch), int(cap)))
    return 1 << (b - 1).bit_length()


# ONE plan cache for every demodulator (PSK and FSK plans, keyed by kind):
# its byte budget (AMR_PLAN_CACHE_BYTES, default 64 GB, 2/9 of an MI355X's
# HBM) bounds all the drop-in path's device memory together.
plan_cache = PlanCache(_cache_budget())
PSK_MAX_CHUNK = 4096


def get_psk_plan(kind: str, n: int, baud, carrier, samp_rate, batch: int) -> PskPlan:
    """Plan cache keyed by the reference call's parameters (and device)."""
    dev = default_device()
    key = ("psk", kind, int(n), float(baud), float(carrier), float(samp_rate), dev)
    need = stream_bucket(batch, PSK_MAX_CHUNK)
    sps = int(samp_rate / baud)
    first = sps if kind == "bpsk" else sps // 2

    def estimate(m):
        return max(0, int(lib().amr_psk_plan_bytes_estimate(psk_kind(kind), int(n), sps, first, 9, 5, m)))
    return plan_cache.get(key, need, lambda m: PskPlan(kind, n, baud, carrier, samp_rate, max_streams=m, device=dev),
                          estimate if sps >= 1 else None)


# ---------------------------------------------------------------------------
# ofdm: the multi-carrier DQPSK modem (tests/ofdm_cases.py)
def ofdm_geometry(baud, carrier, num_subcarriers, samp_rate=96000):
    """(sps, L, Ncp, Nu, bins int32 [K]) of DESIGN.md §3j, or ValueError when the
    geometry is not valid (host arithmetic, before any device work)."""
    K = int(num_subcarriers)
    sps = int(samp_rate / baud)
    if not 1 <= K <= OFDM_MAX_K:
        raise ValueError(f"ofdm: num_subcarriers {K} outside [1, {OFDM_MAX_K}]")
    if sps < 1:
        raise ValueError("ofdm: fewer than one sample per dibit")
    L = K * sps
    Ncp = L // 8
    Nu = L - Ncp
    c0 = int(np.floor(float(carrier) * Nu / float(samp_rate) + 0.5))
    bins = c0 - K // 2 + np.arange(K, dtype=np.int64)
    if bins[0] < 1:
        raise ValueError(f"ofdm: lowest subcarrier on bin {int(bins[0])}, below bin 1")
    if 2 * bins[-1] >= Nu:
        raise ValueError(f"ofdm: highest subcarrier on bin {int(bins[-1])}, at or above Nu / 2 = {Nu} / 2")
    return sps, L, Ncp, Nu, bins.astype(np.int32)


def design_ofdm(baud, carrier, num_subcarriers, samp_rate=96000):
    """The geometry and the twiddle table W [K][Nu][2] float64, (cos th, -sin th)
    with th = (2 pi) * (((bins[k] * m) % Nu) / Nu): what the plan takes, and what
    tests/ofdm_cases.py correlates against."""
    sps, L, Ncp, Nu, bins = ofdm_geometry(baud, carrier, num_subcarriers, samp_rate)
    r = (bins.astype(np.int64)[:, None] * np.arange(Nu, dtype=np.int64)[None, :]) % Nu
    th = (2 * np.pi) * (r / Nu)
    W = np.ascontiguousarray(np.stack([np.cos(th), -np.sin(th)], axis=-1), np.float64)
    return sps, L, Ncp, Nu, bins, W


def _rows(x: np.ndarray):
    """(x, row stride in elements): rows of a wider array go as they are."""
    B, n = x.shape
    if x.strides[1] != x.itemsize or (B > 1 and (x.strides[0] % x.itemsize or x.strides[0] < n * x.itemsize)):
        x = np.ascontiguousarray(x)
    return x, (x.strides[0] // x.itemsize if B > 1 else n)


class _SymPlan:
    """What the symbol modems' plans (OfdmPlan, DsssPlan, MskPlan) share, over the amr_<_abi>_* entries: the handle's
    lifetime, the batching of a call into max_streams streams at a time, the host demodulation and stage
    loops, and the plan accessors.  A subclass sets _abi and _slots and calls _create from its __init__."""
    _abi = ""
    _slots = ()

    def _fn(self, name):
        return getattr(lib(), f"amr_{self._abi}_{name}")

    def _create(self, device, max_streams, *design):
        """amr_<_abi>_plan_create(&handle, device, *design, max_streams)"""
        require_gpu()
        self.device = default_device() if device is None else device
        self.max_streams = int(max_streams)
        h = ctypes.c_void_p()
        check(self._fn("plan_create")(ctypes.byref(h), self.device, *design, self.max_streams))
        self.handle = h
        self.out_cap = int(self._fn("plan_out_capacity")(h))
        self.lock = threading.Lock()

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and _lib is not None:
            try:
                getattr(_lib, f"amr_{self._abi}_plan_destroy")(h)
            except Exception:
                pass
            self.handle = None

    def _batches(self, x):
        x, stride = _rows(x)
        for s0 in range(0, x.shape[0], self.max_streams):
            yield s0, x[s0:s0 + self.max_streams], stride

    def _demod(self, x, entry, soft, tail):
        """A host demodulation entry on x, max_streams streams at a time: (list[bytes], sync, list[int8 array]
        or None, offsets int64 [B]).  tail(sv, of): the entry's arguments after sync_idx, from sv = (soft
        or NULL, soft_stride) and the batch's offsets array `of` (left zero where the entry has none)."""
        outs, softs = [], []
        syncs, offs = np.empty(x.shape[0], np.int64), np.zeros(x.shape[0], np.int64)
        cap = max(self.out_cap, 1)
        for s0, xb, stride in self._batches(x):
            nb = xb.shape[0]
            out = np.empty((nb, cap), np.uint8)
            sv = np.empty((nb, 8 * cap), np.int8) if soft else None
            ln, sy, of = np.empty(nb, np.int64), np.empty(nb, np.int64), offs[s0:s0 + nb]
            with self.lock:
                check(self._fn(entry)(self.handle, ptr(xb), DTYPES[xb.dtype], nb, stride, ptr(out), cap, ptr(ln),
                                      ptr(sy), *tail((ptr(sv) if soft else None, 8 * cap), of)))
            outs += [out[i, :ln[i]].tobytes() for i in range(nb)]
            if soft:
                softs += [sv[i, :8 * ln[i]].copy() for i in range(nb)]
            syncs[s0:s0 + nb] = sy
        return outs, syncs, (softs if soft else None), offs

    def _stage(self, x, entry, outs, offsets=None):
        """A stage entry on x, max_streams streams at a time: entry(plan, x, dtype, B, x_stride[, offsets],
        *outs), each of `outs` a C-contiguous [B][...] array the batches fill; returns outs."""
        for s0, xb, stride in self._batches(x):
            nb = xb.shape[0]
            ob = None if offsets is None else np.ascontiguousarray(offsets[s0:s0 + nb])
            with self.lock:
                check(self._fn(entry)(self.handle, ptr(xb), DTYPES[xb.dtype], nb, stride,
                                      *(() if ob is None else (ptr(ob),)), *(ptr(o[s0:s0 + nb]) for o in outs)))
        return outs

    def scratch_bytes(self) -> int:
        """Device bytes this plan holds (tables, Y, words + host-API staging + the acquisition buffers once used)."""
        return int(self._fn("plan_scratch_bytes")(self.handle)) if self.handle else 0

    def enable_timing(self, on=True):
        check(self._fn("plan_enable_timing")(self.handle, 1 if on else 0))

    def synchronize(self):
        check(self._fn("plan_synchronize")(self.handle))

    def timings(self) -> dict:
        ms = (ctypes.c_float * len(self._slots))()
        check(self._fn("plan_timings")(self.handle, ms, len(self._slots)))
        return {k: float(v) for k, v in zip(self._slots, ms) if v >= 0}


def _plan_acquires(pl, key, nbytes):
    """A cached plan about to acquire: the first time, the cache makes room for its acquisition
    buffers (nbytes(): the modem's amr_*_acquire_bytes_estimate)."""
    if not getattr(pl, "acquires", False):
        plan_cache.reserve(key, max(0, int(nbytes())))
        pl.acquires = True


class OfdmPlan(_SymPlan):
    """A device plan of the ofdm demodulator: W in HBM + Y and the bit words for max_streams streams."""
    _abi = "ofdm"
    _slots = TO_SLOTS

    def __init__(self, n: int, baud, carrier, num_subcarriers, samp_rate=96000, max_streams=64, device=None):
        self.n, self.baud, self.carrier, self.samp_rate = int(n), baud, carrier, samp_rate
        self.sps, self.L, self.Ncp, self.Nu, self.bins, W = design_ofdm(baud, carrier, num_subcarriers, samp_rate)
        self.K = len(self.bins)
        self.S = self.n // self.L
        self._create(device, max_streams, self.n, self.sps, self.K, ptr(self.bins), ptr(W))

    def demod_host(self, x: np.ndarray, acquire=False):
        """x [B][N] float32 / float64 / int16 (PCM, read as int16 / 32768).  Returns (list[bytes], sync);
        acquire=True: each stream from its own acquired offset, (list[bytes], sync, offsets)."""
        if acquire:
            outs, syncs, _, offs = self.demod_acq_host(x)
            return outs, syncs, offs
        return self._demod(x, "demod_host", False, lambda sv, of: ())[:2]

    def demod_soft_host(self, x: np.ndarray, acquire=False):
        """demod_host with the soft values: (list[bytes], sync, list[int8 array]);
        soft[i][j] belongs to bit j of outs[i].  acquire=True: the offsets as a fourth value."""
        if acquire:
            return self.demod_acq_host(x, soft=True)
        return self._demod(x, "demod_soft_host", True, lambda sv, of: sv)[:3]

    def symbols(self, x: np.ndarray) -> np.ndarray:
        """The DFT stage alone (amr_ofdm_symbols_host): Y [B][S][K] complex128."""
        Y, = self._stage(x, "symbols_host", [np.zeros((x.shape[0], self.S, self.K, 2))])
        return Y.view(np.complex128)[..., 0]

    def demod_acq_host(self, x: np.ndarray, soft=False):
        """Acquisition, then the demodulation of every stream from its offset (amr_ofdm_demod_acq_host):
        (list[bytes], sync, list[int8 array] or None, offsets int64 [B])."""
        return self._demod(x, "demod_acq_host", soft, lambda sv, of: (*sv, ptr(of)))

    def acquire(self, x: np.ndarray):
        """The acquisition stage alone (amr_ofdm_acquire_host): (offset int64 [B], dhat int64 [B], E float64 [B][L])."""
        B = x.shape[0]
        return tuple(self._stage(x, "acquire_host", [np.empty(B, np.int64), np.empty(B, np.int64),
                                                     np.empty((B, self.L))]))

    def symbols_at(self, x: np.ndarray, offsets) -> np.ndarray:
        """The DFT stage at given per-stream offsets (amr_ofdm_symbols_at_host): Y [B][S][K] complex128."""
        Y, = self._stage(x, "symbols_at_host", [np.zeros((x.shape[0], self.S, self.K, 2))],
                         np.ascontiguousarray(offsets, np.int64))
        return Y.view(np.complex128)[..., 0]


def get_ofdm_plan(n: int, baud, carrier, num_subcarriers, samp_rate, batch: int, acquire=False) -> OfdmPlan:
    """The shared plan cache, keyed by the call's parameters (and device).  acquire: the plan is about to
    acquire; the first time, the cache makes room for its acquisition buffers (amr_ofdm_acquire_bytes_estimate)."""
    dev = default_device()
    K = int(num_subcarriers)
    key = ("ofdm", int(n), float(baud), float(carrier), K, float(samp_rate), dev)
    need = stream_bucket(batch, PSK_MAX_CHUNK)
    sps, *_ = ofdm_geometry(baud, carrier, K, samp_rate)                # ValueError before any plan is evicted

    def estimate(m):
        return max(0, int(lib().amr_ofdm_plan_bytes_estimate(int(n), sps, K, m)))
    pl = plan_cache.get(key, need, lambda m: OfdmPlan(n, baud, carrier, K, samp_rate, max_streams=m, device=dev),
                        estimate)
    if acquire:
        _plan_acquires(pl, key, lambda: lib().amr_ofdm_acquire_bytes_estimate(int(n), sps, K, pl.max_streams))
    return pl


def ofdm_tx_samples(n_bytes: int, baud, carrier, num_subcarriers, samp_rate=96000) -> int:
    """len() of ofdm_modulate's output for an n_bytes payload: (1 + ceil((40 + 4 n) / K)) * L."""
    _, L, _, _, bins = ofdm_geometry(baud, carrier, num_subcarriers, samp_rate)
    K = len(bins)
    return (1 + -(-(40 + 4 * int(n_bytes)) // K)) * L


def ofdm_modulate(datas, baud, carrier, num_subcarriers, samp_rate=96000, n_out=None, pcm=False):
    """Batched ofdm modulator on the GPU (amr_ofdm_modulate_host): [B][n_out]
    float32, cut / zero-padded to n_out (default: the longest natural length);
    pcm=True also returns wav_from_array's int16."""
    K = int(num_subcarriers)
    natural = [ofdm_tx_samples(len(d), baud, carrier, K, samp_rate) for d in datas]    # the geometry's ValueError
    ofdm_geometry(baud, carrier, K, samp_rate)
    require_gpu()
    if n_out is None:
        n_out = max(natural, default=0)
    check(lib().amr_set_device(default_device()))
    rc, res = _modulate_call(datas, n_out, pcm, lambda *a: lib().amr_ofdm_modulate_host(
        float(baud), float(carrier), float(samp_rate), K, *a))
    check(rc)
    return res


def _slice_bits(B: int, nbits: int, call) -> np.ndarray:
    """A *_slice_host entry's words as bits: call(words) fills uint32 [B][max(1, ceil(nbits / 32))], MSB
    first; the first nbits of every row come back as uint8."""
    words = np.zeros((B, max(1, (nbits + 31) // 32)), np.uint32)
    check(call(ptr(words)))
    return np.unpackbits(words.astype(">u4").view(np.uint8).reshape(B, -1), axis=1)[:, :nbits]


def ofdm_slice(Y: np.ndarray) -> np.ndarray:
    """The slicer stage alone on the GPU (k_ofdm_slice): Y [B][S][K] complex128 ->
    the decided bits [B][2 K (S - 1)] as uint8."""
    require_gpu()
    Y = np.ascontiguousarray(Y, np.complex128)
    B, S, K = Y.shape
    return _slice_bits(B, max(0, 2 * K * (S - 1)), lambda w: lib().amr_ofdm_slice_host(ptr(Y), B, S, K, w))


def ofdm_soft(Y: np.ndarray) -> np.ndarray:
    """The soft stage alone on the GPU (k_ofdm_slice then k_ofdm_soft): Y [B][S][K]
    complex128 -> int8 [B][2 K (S - 1)], one value per decided bit from bit 0."""
    require_gpu()
    Y = np.ascontiguousarray(Y, np.complex128)
    B, S, K = Y.shape
    soft = np.zeros((B, max(0, 2 * K * (S - 1))), np.int8)
    check(lib().amr_ofdm_soft_host(ptr(Y), B, S, K, ptr(soft)))
    return soft


# ---------------------------------------------------------------------------
# spread: the direct-sequence DBPSK modem (tests/spread_cases.py)
def _dsss_code(code) -> np.ndarray:
    c = np.asarray(DSSS_CODE if code is None else code)
    if c.ndim != 1 or not 2 <= c.size <= DSSS_MAX_C:
        raise ValueError(f"spread: a code of {c.size if c.ndim == 1 else c.shape} chips, outside [2, {DSSS_MAX_C}]")
    if not np.all((c == 0) | (c == 1)):
        raise ValueError("spread: every code entry must be 0 or 1")
    return c.astype(np.int64)


def dsss_geometry(baud, carrier, code=None, samp_rate=96000):
    """(spc, L, cyc, code int64 [C]) of DESIGN.md §3l, or ValueError when the
    geometry is not valid (host arithmetic, before any device work).  baud is the chip rate."""
    c = _dsss_code(code)
    spc = int(samp_rate / baud)
    if spc < 1:
        raise ValueError("spread: fewer than one sample per chip")
    L = c.size * spc
    if L > 1 << 24:
        raise ValueError(f"spread: {L} samples per bit, more than 2^24")
    cyc = int(np.floor(float(carrier) * L / float(samp_rate) + 0.5))
    if cyc < 1:
        raise ValueError("spread: less than one carrier cycle per bit")
    if 2 * cyc >= L:
        raise ValueError(f"spread: {cyc} carrier cycles in a bit of {L} samples, at or above half the sample rate")
    return spc, L, cyc, c


def design_dsss(baud, carrier, code=None, samp_rate=96000):
    """The geometry and the tables over i = 0 .. L-1, th = (2 pi) * (((cyc * i) % L) / L):
    Wc [L][2] = (cos th, -sin th), T [L][2] = sg * Wc, Sn [L] = sin th, cs [C] = 1.0 - 2.0 * code;
    what the plan and the modulator take, and what tests/spread_cases.py correlates against."""
    spc, L, cyc, c = dsss_geometry(baud, carrier, code, samp_rate)
    i = np.arange(L, dtype=np.int64)
    th = (2 * np.pi) * (((cyc * i) % L) / L)
    Wc = np.ascontiguousarray(np.stack([np.cos(th), -np.sin(th)], axis=-1), np.float64)
    Sn = np.ascontiguousarray(np.sin(th), np.float64)
    cs = 1.0 - 2.0 * c.astype(np.float64)
    sg = cs[i // spc]
    T = np.ascontiguousarray(sg[:, None] * Wc, np.float64)
    return spc, L, cyc, c, Wc, T, Sn, cs


class DsssPlan(_SymPlan):
    """A device plan of the spread demodulator: the tables in HBM + Y and the bit words for max_streams streams."""
    _abi = "dsss"
    _slots = TD_SLOTS

    def __init__(self, n: int, baud, carrier, code=None, samp_rate=96000, max_streams=64, device=None):
        self.n, self.baud, self.carrier, self.samp_rate = int(n), baud, carrier, samp_rate
        self.spc, self.L, self.cyc, self.code, Wc, T, _, cs = design_dsss(baud, carrier, code, samp_rate)
        self.C = int(self.code.size)
        self.S = self.n // self.L
        self._create(device, max_streams, self.n, self.spc, self.C, self.cyc, ptr(Wc), ptr(T), ptr(cs))

    def demod_host(self, x: np.ndarray, soft=False, acquire=True):
        """x [B][N] float32 / float64 / int16 (PCM, read as int16 / 32768).  Returns (list[bytes], sync,
        list[int8 array] or None, offsets int64 [B]); acquire: each stream from its own acquired offset."""
        return self._demod(x, "demod_host", soft, lambda sv, of: (*sv, ptr(of), 1 if acquire else 0))

    def acquire(self, x: np.ndarray):
        """The acquisition stage alone (amr_dsss_acquire_host): (offset int64 [B], P float64 [B][L])."""
        B = x.shape[0]
        return tuple(self._stage(x, "acquire_host", [np.empty(B, np.int64), np.empty((B, self.L))]))

    def symbols_at(self, x: np.ndarray, offsets=None) -> np.ndarray:
        """The despreader alone at given per-stream offsets, default zeros (amr_dsss_symbols_at_host):
        Y [B][S] complex128."""
        offsets = np.zeros(x.shape[0], np.int64) if offsets is None else np.ascontiguousarray(offsets, np.int64)
        Y, = self._stage(x, "symbols_at_host", [np.zeros((x.shape[0], self.S, 2))], offsets)
        return Y.view(np.complex128)[..., 0]


def get_dsss_plan(n: int, baud, carrier, code, samp_rate, batch: int, acquire=False) -> DsssPlan:
    """The shared plan cache, keyed by the call's parameters, the code among them (and device).  acquire: the
    plan is about to acquire; the first time, the cache makes room for its acquisition buffers."""
    dev = default_device()
    spc, L, cyc, c = dsss_geometry(baud, carrier, code, samp_rate)      # ValueError before any plan is evicted
    C = int(c.size)
    key = ("dsss", int(n), float(baud), float(carrier), tuple(int(v) for v in c), float(samp_rate), dev)
    need = stream_bucket(batch, PSK_MAX_CHUNK)

    def estimate(m):
        return max(0, int(lib().amr_dsss_plan_bytes_estimate(int(n), spc, C, m)))
    pl = plan_cache.get(key, need, lambda m: DsssPlan(n, baud, carrier, c, samp_rate, max_streams=m, device=dev),
                        estimate)
    if acquire:
        _plan_acquires(pl, key, lambda: lib().amr_dsss_acquire_bytes_estimate(int(n), spc, C, pl.max_streams))
    return pl


def dsss_tx_samples(n_bytes: int, baud, carrier, code=None, samp_rate=96000) -> int:
    """len() of spread_modulate's output for an n_bytes payload: (81 + 8 n) * L."""
    return (81 + 8 * int(n_bytes)) * dsss_geometry(baud, carrier, code, samp_rate)[1]


def dsss_modulate(datas, baud, carrier, code=None, samp_rate=96000, n_out=None, pcm=False):
    """Batched spread modulator on the GPU (amr_dsss_modulate_host): [B][n_out]
    float32, cut / zero-padded to n_out (default: the longest natural length);
    pcm=True also returns wav_from_array's int16."""
    spc, L, cyc, c, _, _, Sn, cs = design_dsss(baud, carrier, code, samp_rate)   # the geometry's ValueError
    require_gpu()
    if n_out is None:
        n_out = max(((81 + 8 * len(d)) * L for d in datas), default=0)
    check(lib().amr_set_device(default_device()))
    rc, res = _modulate_call(datas, n_out, pcm, lambda *a: lib().amr_dsss_modulate_host(
        spc, int(c.size), cyc, ptr(cs), ptr(Sn), *a))
    check(rc)
    return res


def dsss_slice(Y: np.ndarray) -> np.ndarray:
    """The slicer stage alone on the GPU (k_dsss_slice): Y [B][S] complex128 -> the decided bits [B][S - 1] as uint8."""
    require_gpu()
    Y = np.ascontiguousarray(Y, np.complex128)
    B, S = Y.shape
    return _slice_bits(B, max(0, S - 1), lambda w: lib().amr_dsss_slice_host(ptr(Y), B, S, w))


def dsss_soft(Y: np.ndarray) -> np.ndarray:
    """The soft stage alone on the GPU (k_dsss_slice then k_dsss_soft): Y [B][S]
    complex128 -> int8 [B][S - 1], one value per decided bit from bit 0."""
    require_gpu()
    Y = np.ascontiguousarray(Y, np.complex128)
    B, S = Y.shape
    soft = np.zeros((B, max(0, S - 1)), np.int8)
    check(lib().amr_dsss_soft_host(ptr(Y), B, S, ptr(soft)))
    return soft


# ---------------------------------------------------------------------------
# minshift: the MSK modem (tests/minshift_cases.py)
def msk_geometry(baud, carrier, samp_rate=96000):
    """(L, h, cyc4) of DESIGN.md §3m, or ValueError when the geometry is not valid (host
    arithmetic, before any device work): L samples per bit, h = L // 2, cyc4 quarter-cycles
    of carrier per bit."""
    L = int(samp_rate / baud)
    if L < 4:
        raise ValueError("minshift: fewer than four samples per bit")
    if L > 1 << 24:
        raise ValueError(f"minshift: {L} samples per bit, more than 2^24")
    cyc4 = int(np.floor(4 * float(carrier) * L / float(samp_rate) + 0.5))
    if cyc4 < 2:
        raise ValueError("minshift: less than half a carrier cycle per bit")
    if cyc4 + 1 >= 2 * L:
        raise ValueError(f"minshift: {cyc4} quarter-cycles in a bit of {L} samples, the upper tone at or above "
                         "half the sample rate")
    return L, L // 2, cyc4


def design_msk(baud, carrier, samp_rate=96000):
    """The geometry and the tables (float64): Sn [4 L] = sin((2 pi) * (p / (4 L)));
    U [L][2] = (cos th, -sin th), th = (2 pi) * (((cyc4 * i) % (4 L)) / (4 L));
    E0, E1 [2 L][2] = (cos th, -sin th), th = (2 pi) * ((((cyc4 -/+ 1) * r) % (2 L)) / (2 L));
    R [L][2] = (cos, +sin)((2 pi) * (d / L)).  What the plan and the modulator take, and what
    tests/minshift_cases.py correlates against."""
    L, h, cyc4 = msk_geometry(baud, carrier, samp_rate)

    def pair(th, sign):
        return np.ascontiguousarray(np.stack([np.cos(th), sign * np.sin(th)], axis=-1), np.float64)
    Sn = np.ascontiguousarray(np.sin((2 * np.pi) * (np.arange(4 * L, dtype=np.int64) / (4 * L))), np.float64)
    i = np.arange(L, dtype=np.int64)
    U = pair((2 * np.pi) * (((cyc4 * i) % (4 * L)) / (4 * L)), -1.0)
    r = np.arange(2 * L, dtype=np.int64)
    E0 = pair((2 * np.pi) * ((((cyc4 - 1) * r) % (2 * L)) / (2 * L)), -1.0)
    E1 = pair((2 * np.pi) * ((((cyc4 + 1) * r) % (2 * L)) / (2 * L)), -1.0)
    R = pair((2 * np.pi) * (i / L), 1.0)
    return L, h, cyc4, Sn, U, E0, E1, R


class MskPlan(_SymPlan):
    """A device plan of the minshift demodulator: the tables in HBM + W and the bit words for max_streams streams."""
    _abi = "msk"
    _slots = TD_SLOTS

    def __init__(self, n: int, baud, carrier, samp_rate=96000, max_streams=64, device=None):
        self.n, self.baud, self.carrier, self.samp_rate = int(n), baud, carrier, samp_rate
        self.L, self.h, self.cyc4, _, U, E0, E1, R = design_msk(baud, carrier, samp_rate)
        self.S = max(0, (self.n + self.h) // self.L - 1)
        self._create(device, max_streams, self.n, self.L, self.cyc4, ptr(U), ptr(E0), ptr(E1), ptr(R))

    def demod_host(self, x: np.ndarray, soft=False, acquire=True):
        """x [B][N] float32 / float64 / int16 (PCM, read as int16 / 32768).  Returns (list[bytes], sync,
        list[int8 array] or None, offsets int64 [B]); acquire: each stream from its own acquired offset."""
        return self._demod(x, "demod_host", soft, lambda sv, of: (*sv, ptr(of), 1 if acquire else 0))

    def acquire(self, x: np.ndarray):
        """The bit-timing stage alone (amr_msk_acquire_host): (offset int64 [B], q complex128 [B])."""
        B = x.shape[0]
        off, q = self._stage(x, "acquire_host", [np.empty(B, np.int64), np.empty((B, 2))])
        return off, q.view(np.complex128)[..., 0]

    def symbols_at(self, x: np.ndarray, offsets=None) -> np.ndarray:
        """The window correlator alone at given per-stream offsets, default zeros (amr_msk_symbols_at_host):
        W [B][Sw] complex128."""
        offsets = np.zeros(x.shape[0], np.int64) if offsets is None else np.ascontiguousarray(offsets, np.int64)
        W, = self._stage(x, "symbols_at_host", [np.zeros((x.shape[0], self.S, 2))], offsets)
        return W.view(np.complex128)[..., 0]


def get_msk_plan(n: int, baud, carrier, shape, samp_rate, batch: int, acquire=False) -> MskPlan:
    """The shared plan cache, keyed by the call's parameters (and device); `shape` is unused (the symbol
    modems' getters share one signature).  acquire: the plan is about to acquire; the first time, the cache
    makes room for its acquisition buffers."""
    dev = default_device()
    L, h, cyc4 = msk_geometry(baud, carrier, samp_rate)                 # ValueError before any plan is evicted
    key = ("msk", int(n), float(baud), float(carrier), float(samp_rate), dev)
    need = stream_bucket(batch, PSK_MAX_CHUNK)

    def estimate(m):
        return max(0, int(lib().amr_msk_plan_bytes_estimate(int(n), L, m)))
    pl = plan_cache.get(key, need, lambda m: MskPlan(n, baud, carrier, samp_rate, max_streams=m, device=dev), estimate)
    if acquire:
        _plan_acquires(pl, key, lambda: lib().amr_msk_acquire_bytes_estimate(int(n), L, pl.max_streams))
    return pl


def msk_tx_samples(n_bytes: int, baud, carrier, samp_rate=96000) -> int:
    """len() of minshift_modulate's output for an n_bytes payload: (82 + 8 n) * L."""
    return (82 + 8 * int(n_bytes)) * msk_geometry(baud, carrier, samp_rate)[0]


def msk_modulate(datas, baud, carrier, samp_rate=96000, n_out=None, pcm=False):
    """Batched minshift modulator on the GPU (amr_msk_modulate_host): [B][n_out]
    float32, cut / zero-padded to n_out (default: the longest natural length);
    pcm=True also returns wav_from_array's int16."""
    L, h, cyc4, Sn, *_ = design_msk(baud, carrier, samp_rate)            # the geometry's ValueError
    require_gpu()
    if n_out is None:
        n_out = max(((82 + 8 * len(d)) * L for d in datas), default=0)
    check(lib().amr_set_device(default_device()))
    rc, res = _modulate_call(datas, n_out, pcm, lambda *a: lib().amr_msk_modulate_host(L, cyc4, ptr(Sn), *a))
    check(rc)
    return res


def msk_offset(c, baud, carrier, samp_rate=96000):
    """The score and maximum stage alone on the GPU (k_msk_acq_max) on given line sums c [B][4] =
    (c0.re, c0.im, c1.re, c1.im), one segment per stream: (offset int64 [B], q complex128 [B])."""
    L, *_, R = design_msk(baud, carrier, samp_rate)
    require_gpu()
    c = np.ascontiguousarray(c, np.float64).reshape(-1, 4)
    off, q = np.zeros(c.shape[0], np.int64), np.zeros((c.shape[0], 2))
    check(lib().amr_set_device(default_device()))
    check(lib().amr_msk_offset_host(L, ptr(R), ptr(c), c.shape[0], ptr(off), ptr(q)))
    return off, q.view(np.complex128)[..., 0]


def msk_slice(W: np.ndarray, cyc4: int) -> np.ndarray:
    """The slicer stage alone on the GPU (k_msk_slice): W [B][Sw] complex128 -> the decided bits [B][Sw - 1] as uint8."""
    require_gpu()
    W = np.ascontiguousarray(W, np.complex128)
    B, S = W.shape
    return _slice_bits(B, max(0, S - 1), lambda w: lib().amr_msk_slice_host(ptr(W), B, S, int(cyc4), w))


def msk_soft(W: np.ndarray, cyc4: int) -> np.ndarray:
    """The soft stage alone on the GPU (k_msk_slice then k_msk_soft): W [B][Sw]
    complex128 -> int8 [B][Sw - 1], one value per decided bit from bit 0."""
    require_gpu()
    W = np.ascontiguousarray(W, np.complex128)
    B, S = W.shape
    soft = np.zeros((B, max(0, S - 1)), np.int8)
    check(lib().amr_msk_soft_host(ptr(W), B, S, int(cyc4), ptr(soft)))
    return soft


# ---------------------------------------------------------------------------
# tone8: the 8-FSK modem with Costas sync (tests/tone8_cases.py)
TONE8_COSTAS = (3, 1, 4, 0, 6, 5, 2)
TONE8_SEARCH = 6                                   # the default search, half tone spacings either way
TONE8_MAX_SEARCH = 16


def tone8_geometry(baud, carrier, samp_rate=96000, search=TONE8_SEARCH):
    """(L, T, c2, G) of DESIGN.md §3n, or ValueError when the geometry is not valid (host
    arithmetic, before any device work): L samples per symbol, T = L // 8 per time slot, c2
    half-cycles of carrier per symbol (tone m has c2 + 2 m), G = search half tone spacings
    looked through either way."""
    G = int(search)
    if G != search or not 0 <= G <= TONE8_MAX_SEARCH:
        raise ValueError(f"tone8: search {search!r} outside 0..{TONE8_MAX_SEARCH}")
    L = int(samp_rate / baud)
    if L < 8 or L % 8:
        raise ValueError(f"tone8: {L} samples per symbol, not a positive multiple of 8")
    if L > 1 << 24:
        raise ValueError(f"tone8: {L} samples per symbol, more than 2^24")
    c2 = int(np.floor(2 * float(carrier) * L / float(samp_rate) + 0.5))
    if c2 - G < 2:
        raise ValueError(f"tone8: {c2} half-cycles of carrier per symbol, the lowest searched line below one cycle")
    if c2 + 14 + G >= L:
        raise ValueError(f"tone8: {c2} half-cycles in a symbol of {L} samples, the highest searched line at or above "
                         "half the sample rate")
    return L, L // 8, c2, G


def design_tone8(baud, carrier, samp_rate=96000, search=TONE8_SEARCH):
    """The geometry and the tables (float64): Sn [2 L] = sin((2 pi) * (p / (2 L)));
    E [2 L][2] = (cos th, -sin th), th = (2 pi) * (r / (2 L)).  What the plan and the modulator
    take, and what tests/tone8_cases.py correlates against."""
    L, T, c2, G = tone8_geometry(baud, carrier, samp_rate, search)
    th = (2 * np.pi) * (np.arange(2 * L, dtype=np.int64) / (2 * L))
    Sn = np.ascontiguousarray(np.sin(th), np.float64)
    E = np.ascontiguousarray(np.stack([np.cos(th), -np.sin(th)], axis=-1), np.float64)
    return L, T, c2, G, Sn, E


def tone8_chunk(search=TONE8_SEARCH) -> int:
    """Start slots one acquisition workgroup takes at this search (amr_tone8_chunk)."""
    v = int(lib().amr_tone8_chunk(int(search)))
    if v < 0:
        check(v)                                   # the AMR_E_* of a search outside 0..16
    return v


class Tone8Plan(_SymPlan):
    """A device plan of the tone8 demodulator: the table in HBM + Y and the bit words for max_streams streams."""
    _abi = "tone8"
    _slots = TD_SLOTS

    def __init__(self, n: int, baud, carrier, samp_rate=96000, search=TONE8_SEARCH, max_streams=64, device=None):
        self.n, self.baud, self.carrier, self.samp_rate = int(n), baud, carrier, samp_rate
        self.L, self.T, self.c2, self.G, _, E = design_tone8(baud, carrier, samp_rate, search)
        self.S = self.n // self.L
        self._create(device, max_streams, self.n, self.L, self.c2, self.G, ptr(E))

    def demod_host(self, x: np.ndarray, soft=False, acquire=True):
        """x [B][N] float32 / float64 / int16 (PCM, read as int16 / 32768).  Returns (list[bytes], sync,
        list[int8 array] or None, start int64 [B], shift int64 [B]); acquire: each stream at its own
        acquired (start, shift), else at (0, 0)."""
        shifts, at = np.zeros(x.shape[0], np.int64), [0]

        def tail(sv, of):
            sh = shifts[at[0]:at[0] + of.size]               # the batches come in order
            at[0] += of.size
            return (*sv, ptr(of), ptr(sh), 1 if acquire else 0)
        return (*self._demod(x, "demod_host", soft, tail), shifts)

    def acquire(self, x: np.ndarray):
        """The acquisition stage alone (amr_tone8_acquire_host): (start int64 [B], shift int64 [B],
        score float64 [B])."""
        B = x.shape[0]
        return tuple(self._stage(x, "acquire_host", [np.empty(B, np.int64), np.empty(B, np.int64), np.empty(B)]))

    def symbols_at(self, x: np.ndarray, offsets=None, shifts=None) -> np.ndarray:
        """The DFT stage alone at given per-stream (offset, shift), default zeros (amr_tone8_symbols_at_host):
        Y [B][S][8] complex128."""
        B = x.shape[0]
        offsets = np.zeros(B, np.int64) if offsets is None else np.ascontiguousarray(offsets, np.int64)
        shifts = np.zeros(B, np.int64) if shifts is None else np.ascontiguousarray(shifts, np.int64)
        Y = np.zeros((B, self.S, 8, 2))
        for s0, xb, stride in self._batches(x):
            nb = xb.shape[0]
            of, sh = np.ascontiguousarray(offsets[s0:s0 + nb]), np.ascontiguousarray(shifts[s0:s0 + nb])
            with self.lock:
                check(self._fn("symbols_at_host")(self.handle, ptr(xb), DTYPES[xb.dtype], nb, stride, ptr(of), ptr(sh),
                                                  ptr(Y[s0:s0 + nb])))
        return Y.view(np.complex128)[..., 0]


def get_tone8_plan(n: int, baud, carrier, shape, samp_rate, batch: int, acquire=False) -> Tone8Plan:
    """The shared plan cache, keyed by the call's parameters, the search (`shape`, None: the default) among
    them (and device).  acquire: the plan is about to acquire; the first time, the cache makes room for its
    acquisition buffers."""
    dev = default_device()
    search = TONE8_SEARCH if shape is None else shape
    L, T, c2, G = tone8_geometry(baud, carrier, samp_rate, search)      # ValueError before any plan is evicted
    key = ("tone8", int(n), float(baud), float(carrier), G, float(samp_rate), dev)
    need = stream_bucket(batch, PSK_MAX_CHUNK)

    def estimate(m):
        return max(0, int(lib().amr_tone8_plan_bytes_estimate(int(n), L, G, m)))
    pl = plan_cache.get(key, need, lambda m: Tone8Plan(n, baud, carrier, samp_rate, G, max_streams=m, device=dev),
                        estimate)
    if acquire:
        _plan_acquires(pl, key, lambda: lib().amr_tone8_acquire_bytes_estimate(int(n), L, G, pl.max_streams))
    return pl


def tone8_tx_samples(n_bytes: int, baud, carrier, samp_rate=96000) -> int:
    """len() of tone8_modulate's output for an n_bytes payload: (7 + ceil(8 n / 3)) * L."""
    return (7 + -(-8 * int(n_bytes) // 3)) * tone8_geometry(baud, carrier, samp_rate, 0)[0]


def tone8_modulate(datas, baud, carrier, samp_rate=96000, n_out=None, pcm=False):
    """Batched tone8 modulator on the GPU (amr_tone8_modulate_host): [B][n_out]
    float32, cut / zero-padded to n_out (default: the longest natural length);
    pcm=True also returns wav_from_array's int16."""
    L, T, c2, G, Sn, _ = design_tone8(baud, carrier, samp_rate, 0)       # the geometry's ValueError
    require_gpu()
    if n_out is None:
        n_out = max(((7 + -(-8 * len(d) // 3)) * L for d in datas), default=0)
    check(lib().amr_set_device(default_device()))
    rc, res = _modulate_call(datas, n_out, pcm, lambda *a: lib().amr_tone8_modulate_host(L, c2, ptr(Sn), *a))
    check(rc)
    return res


def tone8_peak(P, T: int, search: int):
    """The score and maximum stage alone on the GPU (k_tone8_peak, k_tone8_acq_max) on given window
    energies P [B][n_win][15 + 2 search]: (start int64 [B], shift int64 [B], score float64 [B])."""
    P = np.ascontiguousarray(P, np.float64)
    B, nw, NB = P.shape
    if NB != 15 + 2 * int(search):
        raise ValueError(f"tone8_peak: {NB} lines, not 15 + 2 * {search}")
    require_gpu()
    start, shift, score = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B)
    check(lib().amr_set_device(default_device()))
    check(lib().amr_tone8_peak_host(int(T), int(search), ptr(P), B, nw, ptr(start), ptr(shift), ptr(score)))
    return start, shift, score


def tone8_slice(Y: np.ndarray) -> np.ndarray:
    """The slicer stage alone on the GPU (k_tone8_slice): Y [B][S][8] complex128 -> the decided bits [B][3 S] as uint8."""
    require_gpu()
    Y = np.ascontiguousarray(Y, np.complex128)
    B, S, _ = Y.shape
    return _slice_bits(B, 3 * S, lambda w: lib().amr_tone8_slice_host(ptr(Y), B, S, w))


def tone8_soft(Y: np.ndarray) -> np.ndarray:
    """The soft stage alone on the GPU (k_tone8_slice then k_tone8_soft): Y [B][S][8]
    complex128 -> int8 [B][3 S], one value per decided bit from bit 0."""
    require_gpu()
    Y = np.ascontiguousarray(Y, np.complex128)
    B, S, _ = Y.shape
    soft = np.zeros((B, 3 * S), np.int8)
    check(lib().amr_tone8_soft_host(ptr(Y), B, S, ptr(soft)))
    return soft


def fec_decode_host(datas):
    """Batched fec.ReedSolomonFEC.decode on the GPU. Returns (list[bytes], crc_ok[list[bool]])."""
    require_gpu()
    datas = [bytes(d) for d in datas]
    n = len(datas)
    if n == 0:
        return [], []
    stride = max(1, max(len(d) for d in datas))
    buf = np.zeros((n, stride), np.uint8)
    ln = np.array([len(d) for d in datas], np.int64)
    for i, d in enumerate(datas):
        buf[i, :len(d)] = np.frombuffer(d, np.uint8)
    out = np.zeros((n, stride), np.uint8)
    out_len = np.zeros(n, np.int64)
    ok = np.zeros(n, np.int32)
    check(lib().amr_set_device(default_device()))
    check(lib().amr_fec_decode_host(ptr(buf), stride, ptr(ln), n, ptr(out), stride, ptr(out_len), ptr(ok)))
    return [out[i, :out_len[i]].tobytes() for i in range(n)], [bool(v) for v in ok]


VITERBI_MAX_LEN = 1 << 24


def is_codeword_len(n: int) -> bool:
    """A byte length the rate-1/2 K=7 encoder can produce (2 n + 2), up to 2^24."""
    return n % 2 == 0 and 2 <= n <= VITERBI_MAX_LEN


def _pad_rows(datas):
    n = len(datas)
    ln = np.array([len(d) for d in datas], np.int64)
    stride = max(1, int(ln.max()))
    buf = np.zeros((n, stride), np.uint8)
    for i, d in enumerate(datas):
        buf[i, :len(d)] = np.frombuffer(d, np.uint8)
    return buf, ln, stride


def conv_encode(datas):
    """Batched fec.ConvolutionalEncoder.encode on the GPU (amr_conv_encode_host): list[bytes]."""
    require_gpu()
    datas = [bytes(d) for d in datas]
    n = len(datas)
    if n == 0:
        return []
    buf, ln, stride = _pad_rows(datas)
    cap = 2 * int(ln.max()) + 2
    out = np.zeros((n, cap), np.uint8)
    out_len = np.zeros(n, np.int64)
    check(lib().amr_set_device(default_device()))
    check(lib().amr_conv_encode_host(ptr(buf), stride, ptr(ln), n, ptr(out), cap, ptr(out_len)))
    return [out[i, :out_len[i]].tobytes() for i in range(n)]


def viterbi_decode(datas):
    """Batched maximum-likelihood decode of the K=7 code on the GPU
    (amr_viterbi_decode_host).  Returns (list[bytes], list[int]): the messages
    and, per codeword, the coded-bit positions in which it differs from the
    codeword of its decoded message."""
    require_gpu()
    datas = [bytes(d) for d in datas]
    n = len(datas)
    if n == 0:
        return [], []
    buf, ln, stride = _pad_rows(datas)
    cap = max(1, stride // 2)
    out = np.zeros((n, cap), np.uint8)
    out_len = np.zeros(n, np.int64)
    metric = np.zeros(n, np.int32)
    check(lib().amr_set_device(default_device()))
    check(lib().amr_viterbi_decode_host(ptr(buf), stride, ptr(ln), n, ptr(out), cap, ptr(out_len), ptr(metric)))
    return [out[i, :out_len[i]].tobytes() for i in range(n)], [int(v) for v in metric]


VITERBI_SOFT_MAX_VALS = (1 << 21) - 4


def is_soft_row_len(n: int) -> bool:
    """A soft row length of the soft-input decoder: the bit stream, 16 k + 12
    values, or a codeword's byte-aligned image, 16 k >= 16 values."""
    return 12 <= n <= VITERBI_SOFT_MAX_VALS and (n % 16 == 12 or n % 16 == 0)


def viterbi_decode_soft(softs):
    """Batched soft-input decode of the K=7 code on the GPU
    (amr_viterbi_decode_soft_host): softs are int8 rows (> 0 bit 1, < 0 bit 0,
    0 an erasure).  Returns (list[bytes], list[int]): the messages and, per
    row, the sum of |value| where it disagrees with the decoded message's codeword."""
    require_gpu()
    softs = [np.ascontiguousarray(s, np.int8).ravel() for s in softs]
    n = len(softs)
    if n == 0:
        return [], []
    ln = np.array([s.size for s in softs], np.int64)
    stride = max(1, int(ln.max()))
    buf = np.zeros((n, stride), np.int8)
    for i, s in enumerate(softs):
        buf[i, :s.size] = s
    cap = max(1, stride // 16)
    out = np.zeros((n, cap), np.uint8)
    out_len = np.zeros(n, np.int64)
    metric = np.zeros(n, np.int32)
    check(lib().amr_set_device(default_device()))
    check(lib().amr_viterbi_decode_soft_host(ptr(buf), stride, 0, ptr(ln), n, ptr(out), cap, ptr(out_len), ptr(metric)))
    return [out[i, :out_len[i]].tobytes() for i in range(n)], [int(v) for v in metric]


RS_MIN_NSYM, RS_MAX_NSYM, RS_MAX_INTERLEAVE = 2, 64, 64


def rs_check_code(nsym, interleave):
    """The Reed-Solomon code's two parameters as ints, or ValueError."""
    nsym, interleave = int(nsym), int(interleave)
    if not RS_MIN_NSYM <= nsym <= RS_MAX_NSYM:
        raise ValueError(f"nsym {nsym} outside [{RS_MIN_NSYM}, {RS_MAX_NSYM}]")
    if not 1 <= interleave <= RS_MAX_INTERLEAVE:
        raise ValueError(f"interleave {interleave} outside [1, {RS_MAX_INTERLEAVE}]")
    return nsym, interleave


def rs_encoded_len(n: int, nsym: int) -> int:
    """n message bytes as ceil(n / (255 - nsym)) blocks with nsym parity bytes each."""
    return n + -(-n // (255 - nsym)) * nsym


def rs_decoded_len(n: int, nsym: int) -> int:
    """The message bytes of a received length, or -1 when it is not valid: 0, or
    a last block (what is left after the full blocks of 255) of at least nsym + 1."""
    if n <= 0:
        return 0 if n == 0 else -1
    nblk = -(-n // 255)
    return n - nblk * nsym if n - 255 * (nblk - 1) >= nsym + 1 else -1


def rs_encode(datas, nsym=32, interleave=1):
    """Batched fec.ReedSolomonCodec.encode on the GPU (amr_rs_encode_host): list[bytes]."""
    nsym, interleave = rs_check_code(nsym, interleave)
    require_gpu()
    datas = [bytes(d) for d in datas]
    n = len(datas)
    if n == 0:
        return []
    buf, ln, stride = _pad_rows(datas)
    cap = max(1, rs_encoded_len(int(ln.max()), nsym))
    out = np.zeros((n, cap), np.uint8)
    out_len = np.zeros(n, np.int64)
    check(lib().amr_set_device(default_device()))
    check(lib().amr_rs_encode_host(ptr(buf), stride, ptr(ln), n, nsym, interleave, ptr(out), cap, ptr(out_len)))
    return [out[i, :out_len[i]].tobytes() for i in range(n)]


def rs_decode(datas, nsym=32, interleave=1, erasures=None):
    """Batched errors-and-erasures decode on the GPU (amr_rs_decode_host).
    erasures: None, or per row None / the erased stream positions.  Returns
    (list[bytes], corrected list[int], failed list[int]); a failed block's
    message bytes are the received ones."""
    nsym, interleave = rs_check_code(nsym, interleave)
    require_gpu()
    datas = [bytes(d) for d in datas]
    n = len(datas)
    if n == 0:
        return [], [], []
    buf, ln, stride = _pad_rows(datas)
    mask = None
    if erasures is not None:
        if len(erasures) != n:
            raise ValueError(f"erasures: {len(erasures)} rows for {n} messages")
        mask = np.zeros((n, stride), np.uint8)
        for i, e in enumerate(erasures):
            if e is None:
                continue
            pos = np.asarray(list(e), np.int64).reshape(-1)
            if pos.size and (pos.min() < 0 or pos.max() >= ln[i]):
                raise ValueError(f"row {i}: erased position outside [0, {int(ln[i])})")
            mask[i, pos] = 1
    cap = max(1, stride)
    out = np.zeros((n, cap), np.uint8)
    out_len = np.zeros(n, np.int64)
    corrected = np.zeros(n, np.int32)
    failed = np.zeros(n, np.int32)
    check(lib().amr_set_device(default_device()))
    check(lib().amr_rs_decode_host(ptr(buf), stride, ptr(ln), ptr(mask) if mask is not None else None, n, nsym,
                                   interleave, ptr(out), cap, ptr(out_len), ptr(corrected), ptr(failed)))
    return ([out[i, :out_len[i]].tobytes() for i in range(n)], [int(v) for v in corrected],
            [int(v) for v in failed])


def psk_soft(kind: str, sym: np.ndarray) -> np.ndarray:
    """The soft stage alone on the GPU (K4a then K4s, amr_psk_soft_host): sym
    [B][S] complex128 -> int8 [B][bits], one value per decided bit from bit 0."""
    require_gpu()
    sym = np.ascontiguousarray(np.atleast_2d(sym), np.complex128)
    B, S = sym.shape
    nbits = max(0, (S - 1) * psk_bits(kind))
    soft = np.zeros((B, nbits), np.int8)
    check(lib().amr_psk_soft_host(psk_kind(kind), ptr(sym), B, S, ptr(soft)))
    return soft


def fft(x: np.ndarray, inverse: bool = False) -> np.ndarray:
    """numpy.fft.fft / ifft along the last axis of a [batch][n] complex array, on the GPU."""
    require_gpu()
    x = np.ascontiguousarray(np.atleast_2d(x), np.complex128)
    out = np.empty_like(x)
    check(lib().amr_fft_c2c_host(ptr(x), ptr(out), x.shape[1], x.shape[0], 1 if inverse else 0, default_device()))
    return out


def hilbert(x: np.ndarray) -> np.ndarray:
    """scipy.signal.hilbert(x) along the last axis of a real [batch][n] array, on the GPU."""
    require_gpu()
    x = np.ascontiguousarray(np.atleast_2d(x), np.float64)
    out = np.empty(x.shape, np.complex128)
    check(lib().amr_hilbert_host(ptr(x), ptr(out), x.shape[1], x.shape[0], default_device()))
    return out


def hilbert_env_exact(x: np.ndarray) -> np.ndarray:
    """np.abs(scipy.signal.hilbert(x)) along the last axis of a real [batch][n]
    array on the GPU, bit for bit (pocketfft's own transforms and numpy's
    complex arithmetic restated -- the FSK exact path's envelope stage)."""
    require_gpu()
    x = np.array(np.atleast_2d(x), np.float64, copy=True, order="C")
    out = np.empty_like(x)
    check(lib().amr_hilbert_env_exact_host(ptr(x), x.shape[1], x.shape[0], ptr(out), default_device()))
    return out


def resample(x: np.ndarray, num: int) -> np.ndarray:
    """scipy.signal.resample(x, num) for real float64 input (1-D, or rows of a
    2-D array resampled along the last axis) on the GPU, bit for bit
    (pocketfft's rfft / irfft restated) -- the resample of
    decoder.decode_wav_file (decoder.py:385-387)."""
    require_gpu()
    a = np.asarray(x)
    if a.dtype != np.float64:
        raise TypeError("resample: float64 input only (decode_wav_file's soundfile data)")
    rows = np.ascontiguousarray(np.atleast_2d(a))
    if rows.ndim != 2 or num < 1 or rows.shape[1] < 1:
        raise ValueError("resample: need 1-D / 2-D input with at least one sample and num >= 1")
    out = np.empty((rows.shape[0], int(num)), np.float64)
    check(lib().amr_resample_host(ptr(rows), rows.shape[1], int(num), rows.shape[0], ptr(out), default_device()))
    return out[0] if a.ndim == 1 else out
