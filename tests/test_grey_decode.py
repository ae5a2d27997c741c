"""Decode grey on the GPU: nhw_dec_batch_device_grey (the grey forms of k_dec_final and k_dec_scaled<2> / <4>, the
one-channel store of nhw_tensor.h), nhw_dec_batch_grey, decode_grey_device / decode_grey and nhw-dec --grey.

Every expected value comes from tests/grey_cases.py: the oracle decoder's luma (scale 1) or section 14's (scales 2, 4) through the ORACLE's
colour matrix at neutral chroma, and tensor elements from tensor_cases' exact-arithmetic value rule.  Everything is compared byte for byte
(tensors: bit pattern for bit pattern); there is no tolerance.  Status and quality are held against the colour decode of the same files.

Every file is 512 x 512, so the small shapes are small batches: 1, 3 and 9 files (at scale 4 a file is four workgroups: 4 and 12 are no
multiples of eight; k_dec_luma_l2q rounds n up to eight), three files of the three quality bands under all 16 formats, the 35 committed files
once a scale.  Outputs are decoded into sentinel-filled buffers: a refused slot and everything behind the last element must stay as they were."""
import ctypes
import os

import numpy as np
import pytest

from tests import nhw_surgery as ns
from tests.grey_cases import (BANDS, COLOUR_CHANNELS, GREY_FORMATS, NHW_E_ARG, NHW_E_FORMAT, REFUSED_GREY_FORMATS, SCALES, assert_grey, c_grey_format,
                              decode_grey, expected_grey, goldens, grey_format)
from tests.support import built_cli, device_arena, golden, run
from tests.tensor_cases import SENTINEL, decode_scaled, expected_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    import nhwcodec_amd
    d = nhwcodec_amd.Decoder(0, max_batch=36)
    yield d
    d.close()


@pytest.fixture(scope="module")
def colour_verdict(dec):
    """status and quality of the colour decode of every committed file"""
    import torch
    _, files = goldens()
    _, st, qq = dec.decode_device(*device_arena(files))
    torch.cuda.synchronize()
    return st.cpu().numpy(), qq.cpu().numpy()


def _colour_status(dec, files):
    import torch
    _, st, qq = dec.decode_device(*device_arena(files))
    torch.cuda.synchronize()
    return st.cpu().numpy(), qq.cpu().numpy()


# ---------------------------------------------------------------- 5: every committed file, as grey bytes
@pytest.mark.parametrize("scale", SCALES)
def test_goldens_grey_bytes(dec, oracle, colour_verdict, scale):
    names, files = goldens()
    assert {int(n[1:3]) for n in names} == set(range(1, 24)), "a committed file of every quality"
    got, st, qq = decode_grey(dec, files, scale)                   # (checks the canary behind the output)
    assert np.array_equal(st, colour_verdict[0]) and np.array_equal(qq, colour_verdict[1]) and not st.any()
    assert [int(q) for q in qq] == [int(n[1:3]) for n in names]
    assert_grey(oracle, got, files, st, scale, what="goldens")


# ---------------------------------------------------------------- 6: formats
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("dtype,layout,rows", GREY_FORMATS)
def test_three_quality_bands_every_format(dec, oracle, dtype, layout, rows, scale):
    files = [golden(n) for n in BANDS]
    fmt = grey_format(dtype, layout, rows)
    got, st, qq = decode_grey(dec, files, scale, fmt)              # (checks the sentinel behind the tensors)
    assert not st.any() and [int(q) for q in qq] == [10, 18, 23]
    assert_grey(oracle, got, files, st, scale, fmt, what="bands")


# ---------------------------------------------------------------- 7: batch sizes
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n", [1, 3, 9])
def test_batch_sizes(dec, oracle, n, scale):
    names, files = goldens()
    files = files[::4][:n]
    assert len(files) == n
    got, st, _ = decode_grey(dec, files, scale)
    assert not st.any()
    assert_grey(oracle, got, files, st, scale, what=f"n = {n}")


# ---------------------------------------------------------------- 8: damaged files among good ones
def _damaged():
    q20 = ns.read(golden("q20_0.nhw"))
    no_chroma = q20.copy()
    no_chroma.s["packet2"] = b""                                                 # the chroma packet alone is damaged: the luma of this file is whole
    return [golden("q10_0.nhw"), golden("q23_0.nhw")[:40],                       # a truncated file
            ns.write(q20, q=0), golden("q20_0.nhw"),                              # a bad header
            ns.write(no_chroma), golden("q18_0.nhw")]


@pytest.mark.parametrize("scale", SCALES)
def test_damaged_files_among_good_ones(dec, oracle, scale):
    files = _damaged()
    cst, cqq = _colour_status(dec, files)
    assert [bool(s) for s in cst] == [False, True, True, False, True, False], "the colour decode refuses the three damaged files"
    assert cst[1] == NHW_E_FORMAT
    got, st, qq = decode_grey(dec, files, scale)
    assert np.array_equal(st, cst), "a grey decode's statuses are the colour decode's"
    assert np.array_equal(qq[st == 0], cqq[cst == 0])
    assert_grey(oracle, got, files, st, scale, what="damaged")     # (a refused file's slot keeps its sentinel)
    fmt = grey_format("float32", "CHW", "reversed")
    got, st, _ = decode_grey(dec, files, scale, fmt)
    assert np.array_equal(st, cst)
    assert_grey(oracle, got, files, st, scale, fmt, what="damaged")


# ---------------------------------------------------------------- 9: one handle, colour and grey batches in turn
def test_one_handle_colour_and_grey_in_turn(oracle):
    """three batches of different content on a fresh handle: the grey plan reads nothing a colour batch left in the chroma buffers, and leaves
    nothing that a colour batch then reads"""
    import nhwcodec_amd
    batches = [[golden("q20_0.nhw"), golden("q10_0.nhw")], [golden("q23_0.nhw"), golden("q17_0.nhw")], [golden("q01_0.nhw"), golden("q19_0.nhw")]]

    def colour(d, files, scale):
        px, st, _ = decode_scaled(d, files, scale)
        assert not st.any()
        for i, f in enumerate(files):
            assert np.array_equal(px[i], expected_bytes(oracle, f, scale)), f"colour, scale {scale}, file {i}"

    def grey(d, files, scale):
        got, st, _ = decode_grey(d, files, scale)
        assert not st.any()
        assert_grey(oracle, got, files, st, scale, what="in turn")

    for scale in SCALES:
        for order in ((colour, grey, colour), (grey, colour, grey)):
            d = nhwcodec_amd.Decoder(0, max_batch=2)
            try:
                for step, files in zip(order, batches):
                    step(d, files, scale)
            finally:
                d.close()


# ---------------------------------------------------------------- 10: forced slice orders
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("mode", [1, 2])
def test_forced_slice_orders(dec, oracle, mode, scale):
    _, files = goldens()
    assert dec.lib.nhw_dec_debug_slice_order(dec.h, mode) == 0
    try:
        got, st, _ = decode_grey(dec, files, scale)
    finally:
        assert dec.lib.nhw_dec_debug_slice_order(dec.h, 0) == 0
    assert not st.any()
    assert_grey(oracle, got, files, st, scale, what=f"mode {mode}")


# ---------------------------------------------------------------- 11: refusals
def test_refusals_launch_nothing(dec):
    """every NHW_E_ARG case of the grey call: it returns before any launch, so the output, the status and the quality stay at their sentinel"""
    import torch
    files = [golden("q23_0.nhw"), golden("q01_0.nhw")]
    arena, offs, lens = device_arena(files)
    out = torch.full((2 * 512 * 512 * 4 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    st = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    qq = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert out.data_ptr() % 16 == 0
    ptr = dict(arena=arena.data_ptr(), offs=offs.data_ptr(), lens=lens.data_ptr(), out=out.data_ptr(), st=st.data_ptr())

    def call(c, scale=1, shift=0, n=2, handle=dec.h, **null):
        p = dict(ptr, **{k: None for k in null})
        rc = dec.lib.nhw_dec_batch_device_grey(handle, p["arena"], p["offs"], p["lens"], n, scale, ctypes.byref(c) if c is not None else None,
                                               None if p["out"] is None else p["out"] + shift, p["st"], qq.data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    def untouched():
        return bool((out == SENTINEL).all()) and bool((st == 0x5A5A5A5A).all()) and bool((qq == 0x5A5A5A5A).all())

    for kw in COLOUR_CHANNELS + REFUSED_GREY_FORMATS:
        assert call(c_grey_format(**kw)) == NHW_E_ARG, kw
        assert dec.lib.nhw_dec_last_error()
        assert untouched(), kw
    good = c_grey_format()
    for c in (good, None):                                         # a format, and the grey bytes
        for scale in (0, 3, 8, -1):
            assert call(c, scale=scale) == NHW_E_ARG and untouched(), scale
        for shift in (1, 2, 4, 8):
            assert call(c, shift=shift) == NHW_E_ARG and untouched(), shift
        assert call(c, n=0) == NHW_E_ARG and call(c, n=dec.max_batch + 1) == NHW_E_ARG and untouched()
        for null in ("arena", "offs", "lens", "out", "st"):
            assert call(c, **{null: True}) == NHW_E_ARG and untouched(), null
        assert call(c, handle=None) == NHW_E_ARG and untouched()
        for scale in SCALES:                                       # a debug stop on the handle
            dec.lib.nhw_dec_debug_stop_after(dec.h, 4)
            try:
                assert call(c, scale=scale) == NHW_E_ARG
            finally:
                dec.lib.nhw_dec_debug_stop_after(dec.h, 0)
            assert untouched(), scale
    # every other entry point goes on refusing NHW_T_GREY
    assert dec.lib.nhw_dec_batch_device_tensor(dec.h, ptr["arena"], ptr["offs"], ptr["lens"], 2, 1, ctypes.byref(good), ptr["out"], ptr["st"], qq.data_ptr(), None) == NHW_E_ARG
    torch.cuda.synchronize()
    assert untouched()
    assert call(good) == 0 and not untouched()                     # ... and the same call with nothing wrong does run


def test_python_argument_errors(dec):
    import torch
    import nhwcodec_amd as na
    a = device_arena([golden("q23_0.nhw")])
    buf = torch.zeros((512 * 512 + 64,), dtype=torch.uint8, device="cuda")
    with pytest.raises(na.NhwError, match="GREY"):
        dec.decode_grey_device(*a, fmt=na.TensorFormat("float32", "CHW", "RGB"))
    with pytest.raises(na.NhwError, match="TensorFormat"):
        dec.decode_grey_device(*a, fmt="float32")
    with pytest.raises(na.NhwError, match="16-byte aligned"):
        dec.decode_grey_device(*a, out=buf[1:])
    with pytest.raises(na.NhwError):
        dec.decode_grey_device(*a, out=buf[:512 * 512 - 16])
    with pytest.raises(na.NhwError):
        dec.decode_grey_device(*a, scale=3)
    with pytest.raises(na.NhwError):
        dec.decode_tensor_device(*a, na.TensorFormat("float32", "CHW", "GREY"))      # the tensor decode takes no grey format
    with pytest.raises(na.NhwError):
        dec.decode_grey([], scale=1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 12: host path and CLI
@pytest.mark.parametrize("scale", SCALES)
def test_host_path_equals_the_device_call(dec, oracle, scale):
    files = [golden(n) for n in BANDS] + [golden("q20_0.nhw")]
    px, qs = dec.decode_grey(files, scale)
    assert px.shape == (4, 512 // scale, 512 // scale) and px.dtype == np.uint8 and qs == [10, 18, 23, 20]
    got, st, _ = decode_grey(dec, files, scale)
    assert not st.any() and np.array_equal(px, got)
    t = dec.timing()                                               # nhw_dec_last_timing describes a grey decode
    assert t.total_ms > 0 and t.recon_ms > 0 and t.total_ms >= t.entropy_ms
    small = type(dec)(0, max_batch=3)                              # more files than max_batch: chunks
    try:
        assert np.array_equal(small.decode_grey(files, scale)[0], px)
    finally:
        small.close()
    import nhwcodec_amd as na
    with pytest.raises(na.NhwError, match="status"):
        dec.decode_grey([files[0], files[1][:40]], scale)


def test_cli_grey(oracle, tmp_path):
    exe = built_cli("nhw-dec")
    src = tmp_path / "in.nhw"
    src.write_bytes(golden("q18_0.nhw"))
    for scale in (1, 2):
        out = tmp_path / f"out{scale}.pgm"
        args = ["--grey", str(src), str(out)] + (["--scale", str(scale)] if scale != 1 else [])
        rc, so, se = run(exe, *args)
        assert rc == 0, (so, se)
        s = 512 // scale
        want = expected_grey(oracle, golden("q18_0.nhw"), scale)[::-1]       # the PGM's rows are top-down
        assert out.read_bytes() == b"P5\n%d %d\n255\n" % (s, s) + want.tobytes()
    rc, _, _ = run(exe, "--scale", "4", "--grey", str(src), str(tmp_path / "o4.pgm"))     # the options in the other order
    assert rc == 0 and (tmp_path / "o4.pgm").read_bytes()[:15] == b"P5\n128 128\n255\n"
    for args in (["--grey", "--batch", str(tmp_path)], ["--batch", str(tmp_path), "--grey"], ["--grey", "--tar", "a.tar", "b.tar"],
                 ["--grey", "--tiles", "1", "1", "stem", "o.bmp"], ["--grey", "--picture", "a.nhwp", "o.bmp"], ["--picture", "a.nhwp", "o.bmp", "--grey"]):
        rc, so, se = run(exe, *args)
        assert rc == 1 and "--grey" in se, (args, rc, so, se)
    assert not os.path.exists(tmp_path / "in.bmp")
    bad = tmp_path / "bad.nhw"
    bad.write_bytes(golden("q18_0.nhw")[:40])
    rc, so, _ = run(exe, "--grey", str(bad), str(tmp_path / "bad.pgm"))
    assert rc == 3 and "Not an .nhw file" in so and not os.path.exists(tmp_path / "bad.pgm")
