"""Grey windows, crops, resamplers and warps, what needs no GPU: the seven symbols and their prototypes, the Python
names and the argument errors they raise before a device is touched, and plan_windows at one byte a pixel as a stand-alone host program
(tests/tile_plan/check_px.cpp), plain and under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.grey_picture_cases import SYMBOLS
from tests.nhw_surgery import can_sanitize
from tests.picture_cases import make_container
from tests.support import ROOT, load_lib

PROTOTYPES = """
int nhw_untile_windows_grey_device(const void *d_tiles, const nhw_region *d_regs, int n_regs, const nhw_window_use *d_uses, int n_uses,
                                   int tile0, int m, int scale, void *stream);
int nhw_resample_grey_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, int filter, const nhw_tensor_format *fmt,
                                       const uint8_t *d_flags, const uint64_t *d_out_addr, void *stream);
int nhw_warp_grey_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                   const nhw_warp *d_warps, const uint64_t *d_out_addr, void *stream);
int nhw_dec_windows_grey(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                         uint8_t *out, const uint64_t *out_off, int32_t *status);
int nhw_dec_windows_grey_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                   const uint64_t *dst_addr, const uint64_t *dst_pitch, int32_t *status);
int nhw_dec_crops_grey_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                 uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr,
                                 int32_t *status, int filter);
int nhw_dec_warps_grey_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                 uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const nhw_warp *warps, const uint64_t *dst_addr,
                                 int32_t *status);
"""
FUNCTIONS = ("resize_grey_to_tensor_device", "warp_grey_to_tensor_device")
METHODS = ("decode_windows_grey", "decode_windows_grey_device", "decode_pictures_grey", "decode_crops_grey_device", "decode_warps_grey_device")
SRC = os.path.join(ROOT, "tests", "tile_plan", "check_px.cpp")


def test_symbols_and_prototypes():
    lib = load_lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()
    hdr = squeeze(open(os.path.join(ROOT, "include", "nhw_hip.h")).read())
    decls = re.split(r"\n(?=int )", PROTOTYPES.strip())
    assert len(decls) == 7
    for decl in decls:
        assert squeeze(decl) in hdr, decl


def test_python_names():
    import nhwcodec_amd as na
    for name in FUNCTIONS:
        assert callable(getattr(na, name)), name
    for name in METHODS:
        assert callable(getattr(na.Decoder, name)), name


@pytest.fixture()
def grey():
    import nhwcodec_amd as na
    return na.TensorFormat("float16", "CHW", "GREY", "reversed", scale=1 / 255, bias=-0.5)


@pytest.fixture()
def colour():
    import nhwcodec_amd as na
    return na.TensorFormat("float16", "CHW", "RGB", "reversed")


@pytest.fixture()
def handle():
    """a Decoder that never saw a device: the argument checks of its methods come before anything of the handle is used"""
    import nhwcodec_amd as na
    return na.Decoder.__new__(na.Decoder)


IDENTITY = [[1, 0, 0], [0, 1, 0]]


def test_a_colour_format_to_a_grey_call_is_refused(handle, colour):
    import torch
    import nhwcodec_amd as na
    pic = [torch.zeros((4, 5), dtype=torch.uint8)]
    box = [make_container(8, 8, [b"\x02abc"])]
    for call in (lambda: na.resize_grey_to_tensor_device(pic, (2, 2), colour),
                 lambda: na.warp_grey_to_tensor_device(pic, [IDENTITY], (2, 2), colour),
                 lambda: handle.decode_crops_grey_device(box, [(0, 0, 0, 4, 4)], (2, 2), colour),
                 lambda: handle.decode_warps_grey_device(box, [0], [IDENTITY], (2, 2), colour)):
        with pytest.raises(na.NhwError, match="GREY"):
            call()


def test_a_grey_format_to_a_colour_call_is_refused(handle, grey):
    import torch
    import nhwcodec_amd as na
    pic = [torch.zeros((4, 5, 3), dtype=torch.uint8)]
    box = [make_container(8, 8, [b"\x02abc"])]
    for call in (lambda: na.resize_to_tensor_device(pic, (2, 2), grey),
                 lambda: na.warp_to_tensor_device(pic, [IDENTITY], (2, 2), grey),
                 lambda: na.pictures_to_tensor_device(pic, grey),
                 lambda: handle.decode_crops_device(box, [(0, 0, 0, 4, 4)], (2, 2), grey),
                 lambda: handle.decode_warps_device(box, [0], [IDENTITY], (2, 2), grey)):
        with pytest.raises(na.NhwError, match="GREY"):
            call()


@pytest.mark.parametrize("fill", [(0, 0, 0), [7], -1, 256, 1.0, True, None, "0"])
def test_fill_must_be_one_byte(handle, grey, fill):
    import torch
    import nhwcodec_amd as na
    with pytest.raises(na.NhwError, match="fill"):
        na.warp_grey_to_tensor_device([torch.zeros((4, 5), dtype=torch.uint8)], [IDENTITY], (2, 2), grey, fill=fill)
    with pytest.raises(na.NhwError, match="fill"):
        handle.decode_warps_grey_device([make_container(8, 8, [b"\x02abc"])], [0], [IDENTITY], (2, 2), grey, fill=fill)


def test_pictures_must_have_two_dimensions(grey):
    import torch
    import nhwcodec_amd as na
    for bad in (torch.zeros((4, 5, 3), dtype=torch.uint8), torch.zeros((4, 5, 1), dtype=torch.uint8), torch.zeros((20,), dtype=torch.uint8),
                np.zeros((4, 5), np.uint8)):
        with pytest.raises(na.NhwError, match=r"\[H, W\]"):
            na.resize_grey_to_tensor_device([bad], (2, 2), grey)
        with pytest.raises(na.NhwError, match=r"\[H, W\]"):
            na.warp_grey_to_tensor_device([bad], [IDENTITY], (2, 2), grey)
    for empty in ([], None, torch.zeros((4, 5), dtype=torch.uint8)):
        with pytest.raises(na.NhwError):
            na.resize_grey_to_tensor_device(empty, (2, 2), grey)


@pytest.mark.parametrize("filter,limit", [("area", 128), ("cubic", 32)])
def test_a_reduction_beyond_a_filters_limit_is_refused(handle, grey, filter, limit):
    import torch
    import nhwcodec_amd as na
    assert {"area": na.AREA_MAX_REDUCTION, "cubic": na.CUBIC_MAX_REDUCTION}[filter] == limit
    wide, tall = torch.zeros((1, 2 * limit + 1), dtype=torch.uint8), torch.zeros((3 * limit + 1, 1), dtype=torch.uint8)
    for pic, size in ((wide, (1, 2)), (tall, (3, 1))):
        with pytest.raises(na.NhwError, match="limit"):
            na.resize_grey_to_tensor_device([pic], size, grey, filter=filter)
    box = [make_container(8000, 8, [b"\x02abc"] * 16)]
    with pytest.raises(na.NhwError, match="limit"):
        handle.decode_crops_grey_device(box, [(0, 0, 0, 2 * limit + 1, 4)], (4, 2), grey, scale=1, filter=filter)
    with pytest.raises(na.NhwError, match="filter"):
        na.resize_grey_to_tensor_device([wide], (1, 2), grey, filter="lanczos")
    with pytest.raises(na.NhwError, match="filter"):
        handle.decode_crops_grey_device(box, [(0, 0, 0, 4, 4)], (2, 2), grey, filter=2)


def test_the_other_argument_errors_of_the_grey_methods(handle, grey):
    import nhwcodec_amd as na
    box = [make_container(8, 8, [b"\x02abc"])]
    for call in (lambda: handle.decode_windows_grey(box, [(0, 0, 0, 1, 1)], 3),
                 lambda: handle.decode_windows_grey_device(box, [(0, 0, 0, 1, 1)], True),
                 lambda: handle.decode_pictures_grey(box, 8),
                 lambda: handle.decode_pictures_grey([], 1),
                 lambda: handle.decode_windows_grey(box, [(0, 0, 0, 1)], 2),
                 lambda: handle.decode_crops_grey_device(box, [(0, 0, 0, 4, 4)], (0, 2), grey),
                 lambda: handle.decode_crops_grey_device(box, [(0, 0, 0, 4, 4)], (2, 2), "float16"),
                 lambda: handle.decode_warps_grey_device(box, [1], [IDENTITY], (2, 2), grey),
                 lambda: handle.decode_warps_grey_device(box, [0], [IDENTITY], (2, 2), grey, border="wrap")):
        with pytest.raises(na.NhwError):
            call()


# ---------------------------------------------------------------- the plan at one byte a pixel
def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mismatches 0" in r.stdout and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_plan_at_one_byte_a_pixel(tmp_path):
    exe = str(tmp_path / "plan_px")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    _run(exe)


def test_plan_at_one_byte_a_pixel_under_the_sanitizers(tmp_path):
    if not can_sanitize():
        pytest.skip("this machine's compiler cannot link a sanitized program")
    exe = str(tmp_path / "plan_px_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    _run(exe)
