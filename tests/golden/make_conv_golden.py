#!/usr/bin/env python3
"""Generate the convolutional-code fixtures by running the REFERENCE's
fec.ConvolutionalEncoder.encode (fec.py:79-111; needs the reference checkout
that make_golden.py imports from; the tests need only the committed data).

Committed output is data only:
  tests/golden/conv.npz            lengths   int64, the message lengths
                                   rand_in   the seeded random messages, end to end
                                   rand_out  their codewords, end to end
                                   zero_out / ff_out / aa_out
                                             the codewords of all-0x00, all-0xFF and
                                             all-0xAA messages of the same lengths
                                   (message i of length n starts at sum(lengths[:i]),
                                   its codeword of 2n + 2 bytes at sum(2 * lengths[:i] + 2))
  tests/golden/conv_manifest.json  the reference call, the seed, the lengths and
                                   the array layout

Run:  python tests/golden/make_conv_golden.py
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (reference import helper)

LENGTHS = list(range(41)) + [63, 64, 65, 255, 2398]
SEED = 20261020
PATTERNS = {"zero": 0x00, "ff": 0xFF, "aa": 0xAA}


def main():
    scratch = tempfile.mkdtemp(prefix="amr_conv_golden_")
    cwd = os.getcwd()
    _, fec, _ = make_golden._import_reference(scratch)
    enc = fec.ConvolutionalEncoder()
    rng = np.random.default_rng(SEED)
    rand_in, outs = [], {k: [] for k in ("rand", *PATTERNS)}
    for n in LENGTHS:
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        rand_in.append(msg)
        outs["rand"].append(enc.encode(msg))
        for name, v in PATTERNS.items():
            outs[name].append(enc.encode(bytes([v]) * n))
    for cws in outs.values():
        assert [len(c) for c in cws] == [2 * n + 2 for n in LENGTHS]
    arrays = {"lengths": np.array(LENGTHS, np.int64), "rand_in": np.frombuffer(b"".join(rand_in), np.uint8)}
    for name, cws in outs.items():
        arrays[f"{name}_out"] = np.frombuffer(b"".join(cws), np.uint8)
    os.chdir(cwd)
    np.savez_compressed(os.path.join(HERE, "conv.npz"), **arrays)
    manifest = {
        "reference": "fec.ConvolutionalEncoder.encode  fec.py:79-111",
        "seed": SEED,
        "lengths": LENGTHS,
        "patterns": PATTERNS,
        "layout": "message i starts at sum(lengths[:i]); its codeword (2 n + 2 bytes) at sum(2 * lengths[:i] + 2)",
        "arrays": {k: int(v.size) for k, v in arrays.items()},
    }
    with open(os.path.join(HERE, "conv_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print("wrote", len(LENGTHS), "lengths,", sum(v.nbytes for v in arrays.values()), "bytes")


if __name__ == "__main__":
    main()
