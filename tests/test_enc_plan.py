"""The encoder's batch planner (nhwcodec_amd/csrc/nhw_enc_plan.h, the text libnhwhip.so compiles) compiled for the host and held against its own
resource table and against the launch sequences of the driver it replaced (tests/enc_plan/check.cpp): every plan of the domain -- 23 qualities x
both compat values x the four (what, timed) pairs of the driver x small and large n x low_parts 1, 2 x every combination of the ten other
switches at stop 0, and every debug stop at every quality and compat under thirteen switch settings -- for its order (no kernel beside or in
front of one that writes what it touches), its events, its shape and what a switch must not change; and the literal sequences.  A second build
runs the same program under the address and undefined-behaviour sanitizers.  No GPU needed."""
import os
import re
import subprocess

import pytest

from tests.nhw_surgery import can_sanitize
from tests.support import ROOT

SRC = os.path.join(ROOT, "tests", "enc_plan", "check.cpp")
HEADER = os.path.join(ROOT, "nhwcodec_amd", "csrc", "nhw_enc_plan.h")

QUALITIES, COMPAT, PAIRS, SIZES, LOW_PARTS = 23, 2, 4, 2, 2
COMBOS = 3 * 3 * 2 ** 8              # low_chroma x pack_fork x the eight on/off switches
STOPS, STOP_SETTINGS = 48, 13        # the default, every switch off, each of the eleven switches changed alone
PLANS = QUALITIES * COMPAT * (PAIRS * SIZES * LOW_PARTS * COMBOS + STOPS * STOP_SETTINGS)
# 11 default orders, 10 single switches at q20 (one of them the in-line order), 6 x low_chroma / lparts, 3 more in-line orders, 3 x compat,
# 2 parts of a batch in sub-batches, every stop at three qualities
PINNED = 11 + 10 + 6 + 3 + 3 + 2 + 3 * STOPS


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mismatches 0" in r.stdout and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"plans (\d+) pinned (\d+) mismatches 0", r.stdout)
    assert m and int(m.group(1)) == PLANS and int(m.group(2)) >= PINNED, r.stdout[-2000:]
    return r.stdout


def test_plans_are_ordered_and_equal_the_pinned_sequences(tmp_path):
    exe = str(tmp_path / "enc_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    _run(exe)


def test_plans_are_ordered_and_equal_the_pinned_sequences_under_the_sanitizers(tmp_path):
    if not can_sanitize():
        pytest.skip("this machine's compiler cannot link a sanitized program")
    exe = str(tmp_path / "enc_plan_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    _run(exe)


def test_header_stands_alone_without_hip():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", HEADER])
