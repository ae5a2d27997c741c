"""The decoder's batch planner (nhwcodec_amd/csrc/nhw_dec_plan.h, the text libnhwhip.so compiles) compiled for the host and held against its own
resource table and against the launch sequences of the driver it replaced (tests/dec_plan/check.cpp): every plan of the domain -- 3 scales x
colour or grey x NHW_DEC_FORK 0 .. 7, and the debug stops 1 .. 11 x the same bits -- for its order (no kernel beside or in front of one that
writes what it touches), its shape, the grey plans' abstinence and what the bits must not change; and the literal sequences.  A second build
runs the same program under the address and undefined-behaviour sanitizers.  No GPU needed."""
import os
import re
import subprocess

import pytest

from tests.nhw_surgery import can_sanitize
from tests.support import ROOT

SRC = os.path.join(ROOT, "tests", "dec_plan", "check.cpp")
HEADER = os.path.join(ROOT, "nhwcodec_amd", "csrc", "nhw_dec_plan.h")


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mismatches 0" in r.stdout and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"plans (\d+) pinned (\d+) mismatches 0", r.stdout)
    assert m and int(m.group(1)) == 3 * 2 * 8 + 11 * 8 and int(m.group(2)) >= 12 + 7 + 8, r.stdout[-2000:]


def test_plans_are_ordered_and_equal_the_pinned_sequences(tmp_path):
    exe = str(tmp_path / "dec_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    _run(exe)


def test_plans_are_ordered_and_equal_the_pinned_sequences_under_the_sanitizers(tmp_path):
    if not can_sanitize():
        pytest.skip("this machine's compiler cannot link a sanitized program")
    exe = str(tmp_path / "dec_plan_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    _run(exe)


def test_header_stands_alone_without_hip():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", HEADER])
