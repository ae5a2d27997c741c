"""Encode grey without a GPU: the rule nhw_grey_luma (nhwcodec_amd/csrc/nhw_grey.h) against the oracle's colour stage on
the replicated all-greys picture and, by a stand-alone program (tests/grey_encode/check.cpp, plain and under AddressSanitizer + UBSan, nothing
preloaded), against the conversion's three-term expressions; TensorFormat.inverted_grey(); the header and the exported symbols; the Python
argument errors that need no device; the refusals of nhw-enc --grey."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.grey_encode_cases import NHW_E_ARG, all_greys, replicated
from tests.nhw_surgery import can_sanitize
from tests.support import ROOT, built_cli, load_lib, run

CSRC = os.path.join(ROOT, "nhwcodec_amd", "csrc")
HEADER = os.path.join(CSRC, "nhw_grey.h")
ENTRIES = ("nhw_grey_luma_table", "nhw_enc_batch_device_grey", "nhw_enc_batch_grey", "nhw_tensor_to_bytes_grey_device", "nhw_enc_batch_device_grey_tensor",
           "nhw_tile_pictures_grey_device", "nhw_enc_pictures_grey")


def test_table_is_the_oracles_colour_stage(oracle):
    """q 1 .. 23, all 256 greys: the luma oracle.color gives on B = G = R, and its U and V are 128 everywhere"""
    import nhwcodec_amd as na
    lib = load_lib()
    px = replicated(all_greys())
    for q in range(1, 24):
        y, u, v = oracle.color(px, q)
        y = y.reshape(512, 512)
        assert (y == y[0]).all() and np.array_equal(y[0, :256], y[0, 256:]), q          # a function of the byte alone
        assert (u == 128).all() and (v == 128).all(), q
        t = na.grey_luma_table(q)
        assert t.dtype == np.int16 and t.shape == (256,) and np.array_equal(t, y[0, :256]), f"quality {q}"
        raw = np.full(256 + 8, 0x5A5A, np.int16)
        assert lib.nhw_grey_luma_table(q, raw.ctypes.data) == 0 and np.array_equal(raw[:256], t) and (raw[256:] == 0x5A5A).all()
        assert np.array_equal(t, np.arange(256)) == (q >= 20), q                        # the identity at 20 .. 23 and not below
        if q <= 16:
            assert t[0] == 16
    raw = np.full(256, 0x5A5A, np.int16)
    for q in (0, 24, -1):
        assert lib.nhw_grey_luma_table(q, raw.ctypes.data) == NHW_E_ARG and (raw == 0x5A5A).all()
    assert lib.nhw_grey_luma_table(20, None) == NHW_E_ARG
    for bad in (0, 24, 20.0, "20", None, True):
        with pytest.raises(na.NhwError):
            na.grey_luma_table(bad)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_rule_matches_the_three_term_expressions(tmp_path, sanitize):
    if sanitize and not can_sanitize():
        pytest.skip("this machine's compiler cannot link and run a sanitized program")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1"] if sanitize else ["-O2"]
    exe = str(tmp_path / "grey_encode_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC,
                           os.path.join(ROOT, "tests", "grey_encode", "check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-2000:]
    for line in ("checked 5888\n", "mismatches 0\n", "chroma not 128: 0\n", "fixed form differs: 0\n", "not the identity from 20 on: 0\n"):
        assert line in p.stdout, p.stdout[-2000:]


def test_header_stands_alone():
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-x", "c++", HEADER], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "hip/hip_runtime.h" not in open(HEADER).read()


def test_header_declares_and_library_exports_every_entry():
    lib = load_lib()
    hdr = open(os.path.join(ROOT, "include", "nhw_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert re.search(rf"\bint {name}\(", hdr), name
    assert re.search(r"#define NHW_GREY_BYTES\s+262144u", hdr)
    import nhwcodec_amd as na
    for name in ("encode_grey_device", "encode_grey", "encode_grey_tensor_device", "encode_pictures_grey"):
        assert hasattr(na.Encoder, name), name
    for name in ("tensor_to_grey_bytes_device", "tile_pictures_grey_device", "grey_luma_table"):
        assert hasattr(na, name), name


def test_inverted_grey_arithmetic_and_refusals():
    import nhwcodec_amd as na
    f = na.TensorFormat("float16", "HWC", "GREY", "file", scale=3.0, bias=-0.75)
    g = f.inverted_grey()
    assert (g.dtype_name, g.layout, g.channels, g.rows) == ("float16", "HWC", "GREY", "file")
    assert np.float32(g.scale[0]) == np.float32(1) / np.float32(3) and np.float32(g.bias[0]) == np.float32(0.75) / np.float32(3)
    assert g.scale == (g.scale[0],) * 3 and g.bias == (g.bias[0],) * 3 and g.c_struct().channels == 2
    m = na.TensorFormat("float32", channels="GREY", mean=0.485, std=0.229).inverted_grey()
    sc, bi = np.float32(1) / (np.float32(255) * np.float32(0.229)), -np.float32(0.485) / np.float32(0.229)
    assert np.float32(m.scale[0]) == np.float32(1) / sc and np.float32(m.bias[0]) == -bi / sc
    z = na.TensorFormat("float32", channels="GREY", scale=2.0, bias=0.0).inverted_grey()
    assert z.bias[0] == 0.0 and not np.signbit(z.bias[0])                                # -0 / 2 is stored as +0
    u = na.TensorFormat("uint8", "HWC", "GREY", "file").inverted_grey()
    assert u.scale[0] == 1.0 and u.bias[0] == 0.0
    for bad in (dict(scale=0.0), dict(scale=1e-45), dict(scale=1e-30, bias=3e38)):
        with pytest.raises(na.NhwError):
            na.TensorFormat("float32", channels="GREY", **bad).inverted_grey()
    with pytest.raises(na.NhwError, match="GREY"):
        na.TensorFormat("float32", "CHW", "RGB").inverted_grey()
    with pytest.raises(na.NhwError, match="grey"):
        f.inverted()


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_round_trip_condition(dtype):
    """section 17's condition, on the one scale and bias: every byte b, sent through the decode rule of a grey format and back through the encode
    rule of its inverse, returns as b when |scale| * 255 fits the type's precision -- for "unit" (scale 1 / 255) and the imagenet constants of
    one channel, in float32 and float16; bfloat16 has 8 significant bits, too few for 256 levels, and is held to an error of at most 1"""
    import nhwcodec_amd as na
    from tests.grey_encode_cases import rule_bytes, to_bits, widen
    for kw in (dict(scale=1 / 255), dict(mean=0.485, std=0.229)):
        f = na.TensorFormat(dtype, "HWC", "GREY", "file", **kw)
        g = f.inverted_grey()
        b = np.arange(256, dtype=np.float32)
        elem = np.float32(b * np.float32(f.scale[0])) if f.bias[0] == 0 else (b.astype(np.float64) * np.float32(f.scale[0]) + np.float32(f.bias[0])).astype(np.float32)
        back = rule_bytes(widen(to_bits(elem, dtype), dtype), g.scale[0], g.bias[0])
        err = np.abs(back.astype(int) - np.arange(256))
        assert err.max() <= (1 if dtype == "bfloat16" else 0), (dtype, kw, int(err.max()))


def test_python_argument_errors_without_a_device():
    import torch
    import nhwcodec_amd as na
    grey = na.TensorFormat("float32", "CHW", "GREY", "reversed")
    colour = na.TensorFormat("float32", "CHW", "RGB", "reversed")
    x = torch.zeros((1, 1, 512, 512))
    for call in (lambda: na.tensor_to_grey_bytes_device(x, colour), lambda: na.tensor_to_grey_bytes_device(x, "float32"),
                 lambda: na.tensor_to_grey_bytes_device(x, grey),                             # not on a GPU
                 lambda: na.tensor_to_grey_bytes_device(torch.zeros((1, 512, 512)), grey),     # no channel axis
                 lambda: na.tensor_to_grey_bytes_device(x.half(), grey),
                 lambda: na.tensor_to_bytes_device(x, grey),                                   # the colour call goes on refusing a grey format
                 lambda: na.tile_pictures_grey_device([]), lambda: na.tile_pictures_grey_device([torch.zeros((4, 4), dtype=torch.uint8)]),
                 lambda: na.tile_pictures_grey_device(torch.zeros((4, 4), dtype=torch.uint8))):
        with pytest.raises(na.NhwError):
            call()
    for bad in ([], [np.zeros((4, 4, 3), np.uint8)], [np.zeros((4, 4), np.float32)], np.zeros((4, 4), np.uint8)):
        with pytest.raises(na.NhwError):
            na.Encoder._host_pictures(bad, "encode_pictures_grey", grey=True)


def test_cli_refusals(tmp_path):
    """--grey with another mode is refused before any file is touched: the input does not exist and is never asked for"""
    exe = built_cli("nhw-enc")
    src, out = str(tmp_path / "missing.pgm"), str(tmp_path / "out.nhw")
    for args in (["--grey", "--batch", str(tmp_path)], ["--batch", str(tmp_path), "--grey"], ["--grey", "--tar", src, out], ["--grey", "--tiles", src, out],
                 ["--grey", "--picture", src, out], ["--picture", "--grey", src, out], ["--grey", "--max-bytes", "5000", src, out],
                 ["--grey", "--min-psnr", "30", src, out], ["--grey", src, out, "--resize", "64x64"], ["--resize", "64x64", "--grey", src, out]):
        rc, so, se = run(exe, *args)
        assert rc == 1 and "--grey" in se and "Could not open" not in so + se, (args, rc, so, se)
        assert not os.path.exists(out)
