"""The decoder's host tile planners (nhwcodec_amd/csrc/nhw_tile_plan.h over nhw_container.h, the text libnhwhip.so compiles) compiled for the
host and held against a model (tests/tile_plan/check.cpp): containers the check writes itself -- pictures of 1 x 1, 513 x 513 and 1300 x 600, and
damaged ones -- hand-written and seeded random rects at scales 1, 2 and 4, with and without merging: the slots and their files byte for byte,
the use table and its prefix table, the descriptors, the per-rect statuses, the tile cap, and nhw_dec_pictures' plan.  A second build runs
the same program under the address and undefined-behaviour sanitizers.  No GPU needed."""
import os
import subprocess

import pytest

from tests.nhw_surgery import can_sanitize
from tests.support import ROOT

SRC = os.path.join(ROOT, "tests", "tile_plan", "check.cpp")
HEADERS = [os.path.join(ROOT, "nhwcodec_amd", "csrc", h) for h in ("nhw_container.h", "nhw_tile_plan.h")]


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mismatches 0" in r.stdout and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_planners_equal_the_model(tmp_path):
    exe = str(tmp_path / "plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    _run(exe)


def test_planners_equal_the_model_under_the_sanitizers(tmp_path):
    if not can_sanitize():
        pytest.skip("this machine's compiler cannot link a sanitized program")
    exe = str(tmp_path / "plan_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    _run(exe)


@pytest.mark.parametrize("header", HEADERS, ids=os.path.basename)
def test_header_stands_alone_without_hip(header):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", header])
