#!/usr/bin/env python3
"""Digests of the REFERENCE's own results on every case of tests/tail_cases.py
(this container only).

  FEC     fec.ReedSolomonFEC().decode (fec.py:34-69): the returned bytes and
          whether it printed its CRC warning
  frames  decoder.parse_fbp_stream_enhanced (decoder.py:142-208): the frames
          and everything it prints
  sync    the tail of modem.qpsk_demodulate (modem.py:243-266) -- join the bits,
          find the pattern, pack the bytes -- evaluated from the reference's
          own syntax tree at run time: the statements from `bit_str = ...` to
          the end of the function, compiled as a function of `bits`.  The bytes
          it returns and its sync_idx.
Nothing of the reference is copied: tail_digests.json holds, per case family,
the number of cases and one SHA-256 over the concatenated results
(tail_cases.*_result_blob).  tests/test_tail_cases.py recomputes the same
digests from the plain restatements in tests/tail_cases.py.

Run:  python tests/golden/make_tail_golden.py        (needs /root/reference)
"""
from __future__ import annotations

import ast
import contextlib
import io
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/ (tail_cases)
sys.path.insert(0, HERE)

import tail_cases as tc  # noqa: E402
from make_golden import REF, _import_reference  # noqa: E402


def reference_sync_tail(modem):
    """qpsk_demodulate's statements from `bit_str = ...` on, as f(bits) -> (bytes, sync_idx)."""
    with open(os.path.join(REF, "modem.py")) as f:
        tree = ast.parse(f.read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "qpsk_demodulate")
    first = next(i for i, st in enumerate(fn.body) if isinstance(st, ast.Assign) and
                 any(isinstance(t, ast.Name) and t.id == "bit_str" for t in st.targets))
    body = fn.body[first:]
    assert isinstance(body[-1], ast.Return)
    ret = ast.parse("def _():\n    return _result, sync_idx").body[0].body[0]
    body = body[:-1] + [ast.Assign(targets=[ast.Name(id="_result", ctx=ast.Store())], value=body[-1].value), ret]
    tail = ast.FunctionDef(name="sync_tail", args=ast.parse("def _(bits): pass").body[0].args, body=body,
                           decorator_list=[], returns=None, type_comment=None)
    mod = ast.fix_missing_locations(ast.Module(body=[tail], type_ignores=[]))
    ns = dict(vars(modem))
    exec(compile(mod, os.path.join(REF, "modem.py"), "exec"), ns)
    return ns["sync_tail"]


def main():
    out_path = os.path.join(HERE, "tail_digests.json")
    scratch = tempfile.mkdtemp(prefix="amr_tail_")
    cwd = os.getcwd()
    modem, fec, decoder = _import_reference(scratch)
    sync_tail = reference_sync_tail(modem)
    families = {}

    for fam, gen in tc.SYNC_FAMILIES.items():
        def blobs(gen=gen):
            for _, row, n, _ in gen():
                out, idx = sync_tail([int(b) for b in row[:n]])
                yield tc.sync_result_blob(bytes(out), int(idx))
        families[fam] = tc.digest(blobs())

    rs = fec.ReedSolomonFEC()
    for v in tc.FEC_VARIANTS:
        def blobs(v=v):
            for _, data in tc.fec_cases(v):
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    out = rs.decode(data)
                yield tc.fec_result_blob(bytes(out), "CRC" in buf.getvalue())
        families["fec_" + v] = tc.digest(blobs())

    for fam, cases in tc.frame_families().items():
        def blobs(cases=cases):
            for _, raw in cases:
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    frames = decoder.parse_fbp_stream_enhanced(raw)
                yield tc.frame_result_blob(frames, buf.getvalue())
        families[fam] = tc.digest(blobs())

    os.chdir(cwd)
    with open(out_path, "w") as f:
        json.dump({"generator": "tests/golden/make_tail_golden.py",
                   "reference": "fec.ReedSolomonFEC.decode (fec.py:34-69), decoder.parse_fbp_stream_enhanced "
                                "(decoder.py:142-208), the tail of modem.qpsk_demodulate (modem.py:243-266)",
                   "families": families}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{sum(v['cases'] for v in families.values())} cases in {len(families)} families -> {out_path}")


if __name__ == "__main__":
    main()
