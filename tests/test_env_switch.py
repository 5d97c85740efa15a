"""csrc/env_switch.h, the one way the host layer reads an environment switch:
a stand-alone program built with the host compiler, run under each value of
the truth table in the header's comment."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "audio-modem-radio_amd", "csrc")
PROGRAM = r'''
#include <cstdio>
#include "env_switch.h"
int main() {
  std::printf("%d %d %d %lld %lld\n", (int)amr::env_on("AMR_T"), (int)amr::env_not_off("AMR_T"), amr::env_tri("AMR_T"),
              (long long)amr::env_int("AMR_T", 8, 65536, 0), (long long)amr::env_int("AMR_T", -5, 5, 1));
}
'''
#        value: (env_on, env_not_off, env_tri, env_int(8..65536, else 0), env_int(-5..5, else 1))
TABLE = {None: (0, 1, -1, 0, 1),
         "": (0, 1, 0, 0, 0),
         "0": (0, 0, 0, 0, 0),
         "1": (1, 1, 1, 0, 1),
         "2": (0, 1, 0, 0, 2),
         "10": (1, 1, 1, 10, 1),            # only the first character switches; out of -5..5
         "65536": (0, 1, 0, 65536, 1),
         "65537": (0, 1, 0, 0, 1),          # out of both ranges
         "-3": (0, 1, 0, 0, -3),
         "yes": (0, 1, 0, 0, 0)}            # atoll of text is 0


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("env_switch")
    src, exe = d / "env_switch_test.cpp", d / "env_switch_test"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("value", list(TABLE), ids=lambda v: "unset" if v is None else repr(v))
def test_env_helpers_follow_their_truth_table(program, value):
    env = {k: v for k, v in os.environ.items() if k != "AMR_T"}
    if value is not None:
        env["AMR_T"] = value
    out = subprocess.run([program], env=env, check=True, capture_output=True, text=True).stdout.split()
    assert tuple(int(v) for v in out) == TABLE[value]
