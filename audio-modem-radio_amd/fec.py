"""fec.py -- drop-in for the reference's fec module; decode runs on the GPU.

  ReedSolomonFEC.encode   fec.py:11-32  (host; transmit side)
  ReedSolomonFEC.decode   fec.py:34-69  -> k_fec_decode (util_kernels.hip)
  ReedSolomonFEC.decode_batch           batched form (one wave per stream)
Despite its name the reference "Reed-Solomon" is parity-XOR triples plus a
CRC32 trailer; that is what is reproduced, bit for bit.
ConvolutionalEncoder.encode (fec.py:79-111) and ViterbiDecoder.decode
(fec.py:126-155) stay host code, byte for byte the reference's -- and the
latter is the reference's stub, which does not invert the encoder.  Beside
them, with no reference counterpart:
  ConvolutionalEncoder.encode_batch     -> k_conv_encode (viterbi_kernels.hip)
  ViterbiDecoder.decode_ml / decode_ml_batch
                                        -> k_viterbi: maximum-likelihood
                                           hard-decision decoding of that code,
                                           one wavefront per codeword
  ViterbiDecoder.decode_soft / decode_soft_batch
                                        -> k_viterbi_soft: the same decoder on
                                           int8 soft decisions, as
                                           modem.qpsk_demodulate_soft gives them
And beside ReedSolomonFEC, which stays the reference's parity stub, the code its
name promises:
  ReedSolomonCodec.encode / encode_batch -> k_rs_encode (rs_kernels.hip)
  ReedSolomonCodec.decode / decode_batch -> k_rs_decode: systematic
                                           RS(255, 255 - nsym) over GF(2^8)
                                           (0x11D, alpha = 2, first root alpha^0),
                                           shortened last block, block interleave,
                                           errors-and-erasures decoding, one
                                           wavefront per block
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

import _amr


class ReedSolomonFEC:
    def __init__(self, nsym=32):
        self.nsym = nsym

    def encode(self, data: bytes) -> bytes:
        """fec.py:11-32: (b1, b2, b1^b2) triples, odd tail padded with 0xFF, CRC32 LE."""
        encoded = bytearray()
        for i in range(0, len(data), 2):
            if i + 1 < len(data):
                b1, b2 = data[i], data[i + 1]
                encoded.extend([b1, b2, b1 ^ b2])
            else:
                encoded.append(data[i])
                encoded.append(0xFF)
        encoded.extend(struct.pack('<I', zlib.crc32(data) & 0xFFFFFFFF))
        return bytes(encoded)

    def decode(self, data: bytes) -> bytes:
        """fec.py:34-69 on the GPU; prints the reference's warning on a CRC mismatch."""
        if len(data) < 4:
            return data
        out, ok = _amr.fec_decode_host([data])
        if not ok[0]:
            print("Aviso: CRC não corresponde - dados podem estar corrompidos")
        return out[0]

    def decode_batch(self, datas, warn: bool = False):
        """Decode many byte strings in one launch. Returns (list[bytes], list[crc_ok])."""
        outs, oks = _amr.fec_decode_host(datas)
        if warn:
            for d, ok in zip(datas, oks):
                if len(d) >= 4 and not ok:
                    print("Aviso: CRC não corresponde - dados podem estar corrompidos")
        return outs, oks


class ReedSolomonError(ValueError):
    """ReedSolomonCodec.decode: a block could not be decoded, or the length is not one of the code."""


class ReedSolomonCodec:
    """Reed-Solomon over GF(2^8) on the GPU (no reference counterpart):
    field polynomial 0x11D, alpha = 2, generator prod (x - alpha^i), i < nsym.
    A message is cut into blocks of 255 - nsym bytes (the last one shorter), each
    followed by nsym parity bytes; a block corrects e errors and f erasures while
    2 e + f <= nsym.  interleave = I > 1 sends groups of I blocks column by
    column, so that a burst of I * (nsym // 2) bytes is still corrected."""

    def __init__(self, nsym=32, interleave=1):
        self.nsym, self.interleave = _amr.rs_check_code(nsym, interleave)

    def encoded_len(self, n: int) -> int:
        return _amr.rs_encoded_len(n, self.nsym)

    def decoded_len(self, n: int) -> int:
        """The message bytes of n received bytes, or -1 when n is not a length of this code."""
        return _amr.rs_decoded_len(n, self.nsym)

    def encode(self, data: bytes) -> bytes:
        return self.encode_batch([data])[0]

    def encode_batch(self, datas):
        """encode() of every element, in one launch: list[bytes]."""
        return _amr.rs_encode(datas, self.nsym, self.interleave)

    def decode(self, data: bytes, erase_pos=None) -> bytes:
        """The message of a received stream; erase_pos: stream positions known to be
        unreliable.  ReedSolomonError when a block fails or the length is not valid."""
        try:
            outs, _, failed = self.decode_batch([data], None if erase_pos is None else [erase_pos],
                                                return_status=True)
        except ValueError as e:
            if isinstance(e, ReedSolomonError):
                raise
            raise ReedSolomonError(str(e)) from None
        if failed[0]:
            raise ReedSolomonError(f"{failed[0]} block(s) could not be decoded")
        return outs[0]

    def decode_batch(self, datas, erasures=None, return_status: bool = False):
        """decode of every element in one launch: list[bytes]; with
        return_status=True also (corrected, failed): per message the bytes the
        decoded blocks changed and the blocks that failed (their message bytes
        are the received ones).  erasures: None, or per message None / the
        erased stream positions."""
        datas = [bytes(d) for d in datas]
        for i, d in enumerate(datas):
            if _amr.rs_decoded_len(len(d), self.nsym) < 0:
                raise ValueError(f"row {i}: {len(d)} bytes is not a length of this code (0, or a last block "
                                 f"of at least {self.nsym + 1} bytes after the full blocks of 255)")
        outs, corrected, failed = _amr.rs_decode(datas, self.nsym, self.interleave, erasures)
        return (outs, corrected, failed) if return_status else outs


class ConvolutionalEncoder:
    """fec.py:72-111 (rate 1/2, K=7, polynomials 171/133 octal)."""

    def __init__(self, constraint_length=7):
        self.constraint_length = constraint_length
        self.g1 = 0b1111001
        self.g2 = 0b1011011

    def encode(self, data: bytes) -> bytes:
        bits = []
        sr = 0
        for byte in data:
            for bp in range(8):
                sr = ((sr << 1) | ((byte >> (7 - bp)) & 1)) & 0x7F
                bits += [bin(sr & self.g1).count('1') % 2, bin(sr & self.g2).count('1') % 2]
        for _ in range(6):
            sr = (sr << 1) & 0x7F
            bits += [bin(sr & self.g1).count('1') % 2, bin(sr & self.g2).count('1') % 2]
        out = bytearray()
        for i in range(0, len(bits), 8):
            v = 0
            for j in range(8):
                if i + j < len(bits):
                    v = (v << 1) | bits[i + j]
            out.append(v)
        return bytes(out)

    def encode_batch(self, datas):
        """encode() of every element, in one launch on the GPU: list[bytes]."""
        return _amr.conv_encode(datas)


class ViterbiDecoder:
    """fec.py:114-155 -- decode() is the reference's stub (it does not invert
    the encoder); decode_ml / decode_ml_batch are the real decoder, on the GPU.
    constraint_length is ignored, as in the reference: the polynomials fix K=7."""

    def __init__(self, constraint_length=7):
        self.constraint_length = constraint_length
        self.g1 = 0b1111001
        self.g2 = 0b1011011
        self.trellis = {}

    def decode(self, data: bytes) -> bytes:
        """The reference's stub, kept for parity: it drops 12 bits and keeps every
        second one.  To invert ConvolutionalEncoder.encode use decode_ml."""
        bits = [(byte >> (7 - i)) & 1 for byte in data for i in range(8)]
        if len(bits) >= 12:
            bits = bits[:-12]
        used = bits[0::2]
        out = bytearray()
        for i in range(0, len(used), 8):
            v = 0
            for j in range(8):
                if i + j < len(used):
                    v = (v << 1) | used[i + j]
            out.append(v)
        return bytes(out)

    def decode_ml(self, data: bytes) -> bytes:
        """The message whose codeword is nearest (Hamming) to `data`, a hard-decision
        codeword of ConvolutionalEncoder.encode: 2 n + 2 bytes give n.  ValueError
        for a length the encoder cannot produce."""
        return self.decode_ml_batch([data])[0]

    def decode_ml_batch(self, datas, return_errors: bool = False):
        """decode_ml of every element in one launch: list[bytes]; with
        return_errors=True also list[int], the coded bits each input differs in
        from the codeword of its decoded message."""
        datas = [bytes(d) for d in datas]
        for i, d in enumerate(datas):
            if not _amr.is_codeword_len(len(d)):
                raise ValueError(f"codeword {i}: {len(d)} bytes is not a length of this code "
                                 f"(even, 2 .. {_amr.VITERBI_MAX_LEN})")
        outs, errs = _amr.viterbi_decode(datas)
        return (outs, errs) if return_errors else outs

    def decode_soft(self, soft) -> bytes:
        """decode_ml for soft decisions: one int8 per coded bit (> 0 bit 1, < 0 bit
        0, |v| the reliability, 0 an erasure), as modem.qpsk_demodulate_soft gives
        them.  Either the bit stream (16 n + 12 values) or the byte-aligned image
        of the codeword (8 (2 n + 2) values, the last byte's high nibble skipped)."""
        return self.decode_soft_batch([soft])[0]

    def decode_soft_batch(self, softs, return_metrics: bool = False):
        """decode_soft of every element in one launch: list[bytes]; with
        return_metrics=True also list[int], the sum of |value| over the positions
        where an input disagrees with the codeword of its decoded message."""
        softs = [np.ascontiguousarray(s, np.int8).ravel() for s in softs]
        for i, s in enumerate(softs):
            if not _amr.is_soft_row_len(s.size):
                raise ValueError(f"soft row {i}: {s.size} values is not a length of this code "
                                 f"(16 k + 12, or 16 k >= 16; at most {_amr.VITERBI_SOFT_MAX_VALS})")
        outs, metrics = _amr.viterbi_decode_soft(softs)
        return (outs, metrics) if return_metrics else outs

    @staticmethod
    def soft_from_bytes(cw: bytes, mag: int = 1):
        """The bit-stream soft form of a hard codeword of ConvolutionalEncoder.encode:
        +mag for a 1, -mag for a 0, 16 n + 12 values (the last byte's low nibble)."""
        a = np.frombuffer(bytes(cw), np.uint8)
        if not _amr.is_codeword_len(a.size) or not 1 <= int(mag) <= 127:
            raise ValueError("soft_from_bytes: a codeword of 2 n + 2 bytes and 1 <= mag <= 127")
        bits = np.concatenate([np.unpackbits(a[:-1]), np.unpackbits(a[-1:])[4:]]).astype(np.int16)
        return ((2 * bits - 1) * int(mag)).astype(np.int8)
