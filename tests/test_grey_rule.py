"""The grey rule without a GPU: nhw_grey_value of nhwcodec_amd/csrc/nhw_grey.h held against the oracle's colour matrix at
neutral chroma for all 23 x 256 inputs by a stand-alone program (tests/grey/check.cpp, plain and under AddressSanitizer + UBSan; nothing is
preloaded), nhw_grey_table through the built library against the same table, the Python face of the one-channel format, and the exported
symbols.  The reference of every comparison is the oracle's nhwo_dec_color (tests/grey_cases.oracle_table), never the library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.grey_cases import NHW_E_ARG, oracle_table
from tests.nhw_surgery import can_sanitize
from tests.support import ROOT, load_lib

CSRC = os.path.join(ROOT, "nhwcodec_amd", "csrc")
HEADER = os.path.join(CSRC, "nhw_grey.h")


def _build_check(tmp_path, sanitize):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1"] if sanitize else ["-O2"]
    obj_c, obj_cpp, exe = (str(tmp_path / n) for n in ("nhwo_dec.o", "check.o", "grey_check"))
    subprocess.check_call(["gcc", "-std=gnu99", "-ffp-contract=off", *flags, "-c", os.path.join(ROOT, "oracle", "nhwo_dec.c"), "-o", obj_c])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, "-c",
                           os.path.join(ROOT, "tests", "grey", "check.cpp"), "-o", obj_cpp])
    subprocess.check_call(["g++", *flags, obj_c, obj_cpp, "-o", exe, "-lm"])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_rule_matches_the_oracle_on_every_input(tmp_path, sanitize):
    if sanitize and not can_sanitize():
        pytest.skip("this machine's compiler cannot link and run a sanitized program")
    p = subprocess.run([_build_check(tmp_path, sanitize)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-2000:]
    assert "checked 5888\n" in p.stdout and "unequal 0\n" in p.stdout and "mismatches 0\n" in p.stdout, p.stdout[-2000:]


def test_header_stands_alone():
    """g++ takes nhw_grey.h with no HIP header and no other include in front of it"""
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-x", "c++", HEADER], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "hip/hip_runtime.h" not in open(HEADER).read()


def test_library_table_is_the_oracles(oracle):
    lib = load_lib()
    for q in range(1, 24):
        t = np.full(256 + 16, 0x5A, np.uint8)
        assert lib.nhw_grey_table(q, t.ctypes.data) == 0
        assert np.array_equal(t[:256], oracle_table(oracle, q)), f"quality {q}"
        assert (t[256:] == 0x5A).all()
        assert (np.diff(t[:256].astype(int)) >= 0).all(), f"quality {q}: not monotone"
        if q >= 20:
            assert np.array_equal(t[:256], np.arange(256)), f"quality {q}: not the identity"
    assert (oracle_table(oracle, 19)[[16, 128, 235]] == (16, 131, 241)).all() and oracle_table(oracle, 10)[128] == 167
    t = np.full(256, 0x5A, np.uint8)
    for q in (0, 24, -1):
        assert lib.nhw_grey_table(q, t.ctypes.data) == NHW_E_ARG and (t == 0x5A).all(), q
    assert lib.nhw_grey_table(20, None) == NHW_E_ARG


def test_python_grey_table(oracle):
    import nhwcodec_amd as na
    for q in (1, 16, 17, 19, 20, 23):
        t = na.grey_table(q)
        assert t.dtype == np.uint8 and t.shape == (256,) and np.array_equal(t, oracle_table(oracle, q))
    for bad in (0, 24, 20.0, "20", None, True):
        with pytest.raises(na.NhwError):
            na.grey_table(bad)


def test_tensor_format_grey():
    import torch
    import nhwcodec_amd as na
    f = na.TensorFormat("float16", "CHW", "GREY", "reversed", scale=1 / 255, bias=-0.5)
    assert f.shape(5, 7) == (1, 5, 7) and na.TensorFormat("uint8", "HWC", "GREY").shape(5, 7) == (5, 7, 1)
    assert f.scale[0] == float(np.float32(1 / 255)) and f.bias[0] == -0.5 and f.dtype is torch.float16
    c = f.c_struct()
    assert (c.dtype, c.layout, c.channels, c.rows, c.reserved) == (1, 1, 2, 1, 0) and c.scale[0] == f.scale[0] and c.bias[0] == -0.5
    g = na.TensorFormat("float32", channels="GREY", mean=0.485, std=0.229)
    assert np.float32(g.scale[0]) == np.float32(1) / (np.float32(255) * np.float32(0.229)) and np.float32(g.bias[0]) == -np.float32(0.485) / np.float32(0.229)
    for kw in (dict(scale=(1, 1, 1)), dict(bias=(0, 0, 0)), dict(mean=(0.5, 0.5, 0.5), std=0.2), dict(mean=0.5, std=(0.2, 0.2, 0.2)), dict(scale=[2.0])):
        with pytest.raises(na.NhwError):
            na.TensorFormat("float32", channels="GREY", **kw)
    with pytest.raises(na.NhwError):
        na.TensorFormat("uint8", channels="GREY", scale=2)
    with pytest.raises(na.NhwError, match="grey"):
        f.inverted()
    assert na.TensorFormat("float32", "CHW", "RGB").c_struct().channels == 1          # the colour formats are what they were
    assert na.TensorFormat("float32", "CHW", "RGB", scale=(1, 2, 3)).inverted().scale == (1.0, 0.5, float(np.float32(1) / np.float32(3)))


def test_symbols_and_header():
    lib = load_lib()
    for name in ("nhw_grey_table", "nhw_dec_batch_device_grey", "nhw_dec_batch_grey"):
        assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "nhw_hip.h")).read()
    for name in ("nhw_grey_table", "nhw_dec_batch_device_grey", "nhw_dec_batch_grey", "NHW_T_GREY"):
        assert re.search(rf"\b{name}\b", hdr), name
    assert dict(re.findall(r"\b(NHW_T_[A-Z0-9_]+) = (\d+)", hdr))["NHW_T_GREY"] == "2"
    import nhwcodec_amd as na
    assert na.TENSOR_GREY == 2 and hasattr(na.Decoder, "decode_grey_device") and hasattr(na.Decoder, "decode_grey")
    assert ctypes.sizeof(na.CTensorFormat) == 44
